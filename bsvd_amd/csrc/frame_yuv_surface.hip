// frame_yuv_surface.hip -- YUV surfaces beyond NV12 / P010 on the device (include/bsvd_hip.h, bsvd_yuv_to_planar / bsvd_planar_to_yuv and
// their _pad / _crop forms): planar 4:2:0 (yuv420p, yuv420p10le), 4:2:2 (uyvy422, yuyv422, nv16, p210le, yuv422p, yuv422p10le) and 4:4:4
// (yuv444p, yuv444p10le) <-> the planar fp32 tensors of the network.  A translation unit of its own: the code objects of frame_yuv.hip
// stay what they were.  Helper kernels on the caller's stream, outside the captured graphs; bandwidth-bound, the fp32 side decides the
// layout of work over lanes (frame_surface_items.h).  One kernel pair serves the plain and the pad / crop entry points: the plain ones are
// the case Hp == H, Wp == W, where no item owns an image and every item is whole.
#include "bsvd_internal.h"
#include "frame_surface_items.h"

namespace bsvd {

template <class F, int LINEAR>
__global__ __launch_bounds__(256) void yuv_to_planar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, SurfGeom g, YuvDecode k, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        yuv_to_planar_item<F, LINEAR>(src, dst, g, k, i);
}

template <class F, int LINEAR>
__global__ __launch_bounds__(256) void planar_to_yuv_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, SurfGeom g, YuvEncode k, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        planar_to_yuv_item<F, LINEAR>(src, dst, g, k, i);
}

// ---------------------------------------------------------------------------------------------
// host side: the ten formats, validation (no device needed), constants in double, dispatch
using F420P   = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_U8>;
using F420P10 = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_LOW10>;
using FUYVY   = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_UYVY, SMP_U8>;
using FYUYV   = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_YUYV, SMP_U8>;
using FNV16   = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_SEMIPLANAR, SMP_U8>;
using FP210   = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>;
using F422P   = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_PLANAR, SMP_U8>;
using F422P10 = SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_PLANAR, SMP_LOW10>;
using F444P   = SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_U8>;
using F444P10 = SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_LOW10>;
enum { N_FORMATS = 10 };

using DecodeKernel = void (*)(const uint8_t *, float *, SurfGeom, YuvDecode, int64_t);
using EncodeKernel = void (*)(const float *, uint8_t *, SurfGeom, YuvEncode, int64_t);
// [format][chroma]; 4:4:4 has no filter: one kernel for both values
#define BSVD_FMT_ROW(K, F) {K<F, 0>, K<F, 1>}
#define BSVD_FMT_ROW444(K, F) {K<F, 0>, K<F, 0>}
static const DecodeKernel kDecode[N_FORMATS][2] = {
    BSVD_FMT_ROW(yuv_to_planar_kernel, F420P), BSVD_FMT_ROW(yuv_to_planar_kernel, F420P10), BSVD_FMT_ROW(yuv_to_planar_kernel, FUYVY),
    BSVD_FMT_ROW(yuv_to_planar_kernel, FYUYV), BSVD_FMT_ROW(yuv_to_planar_kernel, FNV16), BSVD_FMT_ROW(yuv_to_planar_kernel, FP210),
    BSVD_FMT_ROW(yuv_to_planar_kernel, F422P), BSVD_FMT_ROW(yuv_to_planar_kernel, F422P10), BSVD_FMT_ROW444(yuv_to_planar_kernel, F444P),
    BSVD_FMT_ROW444(yuv_to_planar_kernel, F444P10)};
static const EncodeKernel kEncode[N_FORMATS][2] = {
    BSVD_FMT_ROW(planar_to_yuv_kernel, F420P), BSVD_FMT_ROW(planar_to_yuv_kernel, F420P10), BSVD_FMT_ROW(planar_to_yuv_kernel, FUYVY),
    BSVD_FMT_ROW(planar_to_yuv_kernel, FYUYV), BSVD_FMT_ROW(planar_to_yuv_kernel, FNV16), BSVD_FMT_ROW(planar_to_yuv_kernel, FP210),
    BSVD_FMT_ROW(planar_to_yuv_kernel, F422P), BSVD_FMT_ROW(planar_to_yuv_kernel, F422P10), BSVD_FMT_ROW444(planar_to_yuv_kernel, F444P),
    BSVD_FMT_ROW444(planar_to_yuv_kernel, F444P10)};

// index into the tables above, or -1 with the field that rules the combination out
static int format_of(const BsvdYuvSurface *s, const char **field)
{
    const bool ten = s->bits == 10, high = s->high_bits != 0;
    switch (s->layout) {
    case BSVD_LAYOUT_PLANAR:
        if (ten && high) { *field = "high_bits = 1 (three-plane 10-bit surfaces carry the code in the low bits)"; return -1; }
        return (s->subsampling == BSVD_SUB_420 ? 0 : s->subsampling == BSVD_SUB_422 ? 6 : 8) + (ten ? 1 : 0);
    case BSVD_LAYOUT_SEMIPLANAR:
        if (s->subsampling != BSVD_SUB_422) { *field = "layout = BSVD_LAYOUT_SEMIPLANAR (4:2:2 only; NV12 / P010 are bsvd_yuv420_*)"; return -1; }
        if (ten && !high) { *field = "high_bits = 0 (p210le carries the code in the high bits)"; return -1; }
        return ten ? 5 : 4;
    default:
        if (s->subsampling != BSVD_SUB_422) { *field = "layout = BSVD_LAYOUT_UYVY / YUYV (4:2:2 only)"; return -1; }
        if (ten) { *field = "bits = 10 (the packed layouts are 8 bit)"; return -1; }
        return s->layout == BSVD_LAYOUT_UYVY ? 2 : 3;
    }
}

struct SurfPlan { SurfGeom g; int fmt; int64_t items, frame_bytes; };

// The surface's own description: enums, the served combinations, pitches, offsets, stride.  H x W is the surface's picture.
static int surface_check(const char *fn, int32_t H, int32_t W, const BsvdYuvSurface *s, SurfPlan *p)
{
    if (s->subsampling < BSVD_SUB_420 || s->subsampling > BSVD_SUB_444) { set_error("%s: surface->subsampling = %d (BSVD_SUB_420 .. BSVD_SUB_444)", fn, s->subsampling); return -3; }
    if (s->layout < BSVD_LAYOUT_PLANAR || s->layout > BSVD_LAYOUT_YUYV) { set_error("%s: surface->layout = %d (BSVD_LAYOUT_PLANAR .. BSVD_LAYOUT_YUYV)", fn, s->layout); return -3; }
    if (s->bits != 8 && s->bits != 10) { set_error("%s: surface->bits = %d (8 or 10)", fn, s->bits); return -3; }
    if (s->high_bits != 0 && s->high_bits != 1) { set_error("%s: surface->high_bits = %d (0 or 1)", fn, s->high_bits); return -3; }
    if (s->bits == 8 && s->high_bits) { set_error("%s: surface->high_bits = 1 with bits = 8 (an 8-bit sample fills its byte)", fn); return -3; }
    if (s->matrix < BSVD_MATRIX_BT601 || s->matrix > BSVD_MATRIX_BT2020) { set_error("%s: surface->matrix = %d (BSVD_MATRIX_BT601 .. BT2020)", fn, s->matrix); return -3; }
    if (s->full_range != 0 && s->full_range != 1) { set_error("%s: surface->full_range = %d (0 or 1)", fn, s->full_range); return -3; }
    if (s->chroma != BSVD_CHROMA_NEAREST && s->chroma != BSVD_CHROMA_LINEAR) { set_error("%s: surface->chroma = %d (BSVD_CHROMA_NEAREST, BSVD_CHROMA_LINEAR)", fn, s->chroma); return -3; }
    if (s->reserved0 != 0) { set_error("%s: surface->reserved0 = %d must be 0", fn, s->reserved0); return -3; }
    if (s->reserved1 != 0) { set_error("%s: surface->reserved1 = %d must be 0", fn, s->reserved1); return -3; }
    if (s->reserved2 != 0) { set_error("%s: surface->reserved2 = %lld must be 0", fn, (long long)s->reserved2); return -3; }
    const char *field = "";
    p->fmt = format_of(s, &field);
    if (p->fmt < 0) { set_error("%s: surface->%s: not one of the served formats", fn, field); return -3; }

    const int sb = s->bits == 10 ? 2 : 1;
    const bool packed = s->layout >= BSVD_LAYOUT_UYVY;
    const int planes = packed ? 1 : s->layout == BSVD_LAYOUT_SEMIPLANAR ? 2 : 3;
    const int64_t cw = s->subsampling == BSVD_SUB_444 ? W : W / 2, ch = s->subsampling == BSVD_SUB_420 ? H / 2 : H;
    const int64_t row_bytes[3] = {packed ? (int64_t)W * 2 : (int64_t)W * sb, s->layout == BSVD_LAYOUT_SEMIPLANAR ? 2 * cw * sb : cw * sb, cw * sb};
    const int64_t rows[3] = {H, ch, ch};
    SurfGeom &g = p->g;
    int64_t end = 0;
    for (int i = 0; i < 3; ++i) {
        if (i >= planes) {
            if (s->pitch[i] != 0) { set_error("%s: surface->pitch[%d] = %d must be 0: the layout has %d plane(s)", fn, i, s->pitch[i], planes); return -3; }
            if (s->offset[i] != 0) { set_error("%s: surface->offset[%d] = %lld must be 0: the layout has %d plane(s)", fn, i, (long long)s->offset[i], planes); return -3; }
            g.pitch[i] = g.off[i] = 0;
            continue;
        }
        g.pitch[i] = s->pitch[i] ? s->pitch[i] : row_bytes[i];
        if (g.pitch[i] < row_bytes[i]) { set_error("%s: surface->pitch[%d] = %d bytes is below the plane's row (%lld bytes)", fn, i, s->pitch[i], (long long)row_bytes[i]); return -3; }
        if (s->offset[i] < 0) { set_error("%s: surface->offset[%d] = %lld must not be negative", fn, i, (long long)s->offset[i]); return -3; }
        g.off[i] = i == 0 || s->offset[i] ? s->offset[i] : g.off[i - 1] + g.pitch[i - 1] * rows[i - 1];
        if (sb == 2) {
            if (g.pitch[i] & 1) { set_error("%s: surface->pitch[%d] = %d must be a multiple of 2 with 16-bit samples", fn, i, s->pitch[i]); return -3; }
            if (g.off[i] & 1) { set_error("%s: surface->offset[%d] = %lld must be a multiple of 2 with 16-bit samples", fn, i, (long long)s->offset[i]); return -3; }
        }
        const int64_t e = g.off[i] + g.pitch[i] * rows[i];
        if (e > end) end = e;
    }
    p->frame_bytes = end;
    g.fstride = s->frame_stride ? s->frame_stride : end;
    if (g.fstride < end) { set_error("%s: surface->frame_stride = %lld bytes is below one frame (%lld bytes)", fn, (long long)s->frame_stride, (long long)end); return -3; }
    if (sb == 2 && (g.fstride & 1)) { set_error("%s: surface->frame_stride = %lld must be a multiple of 2 with 16-bit samples", fn, (long long)s->frame_stride); return -3; }
    return 0;
}

// the picture sizes a subsampling can carry (the pad / crop entry points and bsvd_yuv_frame_bytes); a value that is no subsampling is
// surface_check's to name
static int picture_check(const char *fn, int32_t H, int32_t W, int sub)
{
    if (sub == BSVD_SUB_420 && (H < 2 || (H & 1))) { set_error("%s: H = %d must be positive and even (4:2:0)", fn, H); return -3; }
    if (sub != BSVD_SUB_420 && H < 2) { set_error("%s: H = %d must be at least 2", fn, H); return -3; }
    if (sub != BSVD_SUB_444 && (W < 2 || (W & 1))) { set_error("%s: W = %d must be positive and even (4:2:0, 4:2:2)", fn, W); return -3; }
    if (sub == BSVD_SUB_444 && W < 2) { set_error("%s: W = %d must be at least 2", fn, W); return -3; }
    return 0;
}

// pad == 0: the plain entry points, H and W multiples of 4.  pad != 0: the pad / crop entry points, the planar tensor Hp x Wp.
static int yuv_surface_check(const char *fn, const void *yuv, const char *yuv_name, const float *planar, const char *planar_name, int32_t frames,
                             int32_t H, int32_t W, const BsvdYuvSurface *s, SurfPlan *p, int pad, int32_t Hp, int32_t Wp)
{
    if (!yuv) { set_error("%s: %s is NULL", fn, yuv_name); return -3; }
    if (!planar) { set_error("%s: %s is NULL", fn, planar_name); return -3; }
    if (!s) { set_error("%s: surface is NULL", fn); return -3; }
    if (frames <= 0) { set_error("%s: frames = %d must be positive", fn, frames); return -3; }
    if (!pad) {
        if (H <= 0 || (H & 3)) { set_error("%s: H = %d must be a positive multiple of 4", fn, H); return -3; }
        if (W <= 0 || (W & 3)) { set_error("%s: W = %d must be a positive multiple of 4", fn, W); return -3; }
    } else {
        if (picture_check(fn, H, W, s->subsampling)) return -3;
        if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
        if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
        if (Hp - H >= H) { set_error("%s: Hp = %d pads H = %d by a whole dimension or more (reflect is defined up to 2 H - 1)", fn, Hp, H); return -3; }
        if (Wp - W >= W) { set_error("%s: Wp = %d pads W = %d by a whole dimension or more (reflect is defined up to 2 W - 1)", fn, Wp, W); return -3; }
        if (s->subsampling == BSVD_SUB_420 && (Hp & 1)) { set_error("%s: Hp = %d must be even (4:2:0)", fn, Hp); return -3; }
        if (Wp & 3) { set_error("%s: Wp = %d must be a multiple of 4 (rows move as float4)", fn, Wp); return -3; }
    }
    const int rc = surface_check(fn, H, W, s, p);
    if (rc) return rc;
    if (s->bits == 10 && ((uintptr_t)yuv & 1)) { set_error("%s: %s must be 2-byte aligned with 16-bit samples", fn, yuv_name); return -3; }
    if ((uintptr_t)planar & 15) { set_error("%s: %s must be 16-byte aligned (rows move as float4)", fn, planar_name); return -3; }
    const int64_t per_frame = (int64_t)(s->subsampling == BSVD_SUB_420 ? H / 2 : H) * items_per_row(W);
    if (per_frame > 0x7fffffff) { set_error("%s: H x W = %d x %d: more than 2^31 items per frame", fn, H, W); return -3; }
    p->items = per_frame * frames;
    p->g.H = H; p->g.W = W; p->g.Hp = pad ? Hp : H; p->g.Wp = pad ? Wp : W; p->g.cc = 0; p->g.const_val = 0.f;
    return 0;
}

// The constants of bsvd_yuv420_to_planar / bsvd_planar_to_yuv420 (frame_yuv.hip: decode_constants, encode_constants), from the surface's
// bits, matrix and range: the same doubles rounded to the same floats, which is what makes yuv420p bit-equal to NV12.
static const double kSurfMatrix[3][2] = {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}};   // (Kr, Kb): BT.601, BT.709, BT.2020 ncl

static YuvDecode surf_decode_constants(const BsvdYuvSurface *s)
{
    const int bits = s->bits;
    const double sc = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kSurfMatrix[s->matrix][0], kb = kSurfMatrix[s->matrix][1], kg = 1.0 - kr - kb;
    YuvDecode k;
    k.y_off = s->full_range ? 0.f : (float)(16 * sc);
    k.y_mul = (float)(1.0 / (s->full_range ? top : 219 * sc));
    k.c_off = s->full_range ? (float)(1 << (bits - 1)) : (float)(128 * sc);
    k.c_mul = (float)(1.0 / (s->full_range ? top : 224 * sc));
    k.r_cr = (float)(2 * (1 - kr));
    k.g_cr = (float)(2 * kr * (1 - kr) / kg);
    k.g_cb = (float)(2 * kb * (1 - kb) / kg);
    k.b_cb = (float)(2 * (1 - kb));
    return k;
}

static YuvEncode surf_encode_constants(const BsvdYuvSurface *s)
{
    const int bits = s->bits;
    const double sc = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kSurfMatrix[s->matrix][0], kb = kSurfMatrix[s->matrix][1], kg = 1.0 - kr - kb;
    const double cs = s->full_range ? top : 224 * sc;
    YuvEncode k;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
    k.y_mul = (float)(s->full_range ? top : 219 * sc);
    k.y_off = s->full_range ? 0.f : (float)(16 * sc);
    k.cb_mul = (float)(cs / (2 * (1 - kb)));
    k.cr_mul = (float)(cs / (2 * (1 - kr)));
    k.c_off = s->full_range ? (float)(1 << (bits - 1)) : (float)(128 * sc);
    k.y_lo = k.c_lo = s->full_range ? 0.f : (float)(16 * sc);
    k.y_hi = s->full_range ? (float)top : (float)(235 * sc);
    k.c_hi = s->full_range ? (float)top : (float)(240 * sc);
    return k;
}

static int decode(const char *fn, const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                  const BsvdYuvSurface *s, int32_t const_channels, float const_value, void *stream)
{
    SurfPlan p;
    const int rc = yuv_surface_check(fn, src, "src", dst, "dst", frames, H, W, s, &p, pad, Hp, Wp);
    if (rc) return rc;
    if (const_channels < 0) { set_error("%s: const_channels = %d must not be negative", fn, const_channels); return -3; }
    p.g.cc = const_channels;
    p.g.const_val = const_value;
    return launch_sweep(kDecode[p.fmt][s->chroma], p.items, stream, (const uint8_t *)src, dst, p.g, surf_decode_constants(s), p.items);
}

static int encode(const char *fn, const float *src, void *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                  const BsvdYuvSurface *s, void *stream)
{
    SurfPlan p;
    const int rc = yuv_surface_check(fn, dst, "dst", src, "src", frames, H, W, s, &p, pad, Hp, Wp);
    if (rc) return rc;
    return launch_sweep(kEncode[p.fmt][s->chroma], p.items, stream, src, (uint8_t *)dst, p.g, surf_encode_constants(s), p.items);
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_yuv_frame_bytes(int32_t H, int32_t W, const BsvdYuvSurface *surface)
{
    SurfPlan p;
    if (!surface) return -1;
    if (picture_check("bsvd_yuv_frame_bytes", H, W, surface->subsampling) || surface_check("bsvd_yuv_frame_bytes", H, W, surface, &p)) return -1;
    return p.frame_bytes;
}

int bsvd_yuv_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvSurface *surface, int32_t const_channels,
                       float const_value, void *stream)
{
    return decode("bsvd_yuv_to_planar", src, dst, frames, H, W, 0, 0, 0, surface, const_channels, const_value, stream);
}

int bsvd_planar_to_yuv(const float *src, void *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvSurface *surface, void *stream)
{
    return encode("bsvd_planar_to_yuv", src, dst, frames, H, W, 0, 0, 0, surface, stream);
}

int bsvd_yuv_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const BsvdYuvSurface *surface,
                           int32_t const_channels, float const_value, void *stream)
{
    return decode("bsvd_yuv_to_planar_pad", src, dst, frames, H, W, 1, Hp, Wp, surface, const_channels, const_value, stream);
}

int bsvd_planar_to_yuv_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvSurface *surface,
                            void *stream)
{
    return encode("bsvd_planar_to_yuv_crop", src, dst, frames, H, W, 1, Hp, Wp, surface, stream);
}

}  // extern "C"
