// frame_yuv.hip -- YUV frame I/O on the device (include/bsvd_hip.h): surfaces as decoders, capture cards and encoders hand them over <-> the
// planar fp32 tensors of the network.  Twelve formats, one kernel pair: NV12 and P010 through bsvd_yuv420_to_planar / bsvd_planar_to_yuv420
// (described by a BsvdYuvDesc), planar 4:2:0 (yuv420p, yuv420p10le), 4:2:2 (uyvy422, yuyv422, nv16, p210le, yuv422p, yuv422p10le) and 4:4:4
// (yuv444p, yuv444p10le) through bsvd_yuv_to_planar / bsvd_planar_to_yuv (described by a BsvdYuvSurface), each with its _pad / _crop form.
// The YUV counterpart of u8_to_planar_kernel / planar_to_u8_kernel (tensor_layout.hip): helper kernels on the caller's stream, outside the
// captured graphs; bandwidth-bound, the fp32 side decides the layout of work over lanes (frame_surface_items.h).  The kernel pair serves
// the plain and the pad / crop entry points alike: the plain ones are the case Hp == H, Wp == W, where no item owns an image and every
// item is whole.  Kernels and tables first, then the BsvdYuvSurface front, then the BsvdYuvDesc front.
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
__global__ __launch_bounds__(256) void planar_to_yuv_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, SurfGeom g, YuvEncode k, Dither di, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        planar_to_yuv_item<F, LINEAR>(src, dst, g, k, di, i);
}

// ---------------------------------------------------------------------------------------------
// host side: the formats, validation (no device needed), constants in double, dispatch
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
using FNV12   = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_U8>;
using FP010   = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>;
// the last two rows are the BsvdYuvDesc front's alone: FMT_NV12 + desc->pix_fmt; format_of never names them
enum { FMT_NV12 = 10, N_FORMATS = 12 };
static_assert(BSVD_PIX_NV12 == 0 && BSVD_PIX_P010 == 1, "FMT_NV12 + pix_fmt indexes the last two table rows");

using DecodeKernel = void (*)(const uint8_t *, float *, SurfGeom, YuvDecode, int64_t);
using EncodeKernel = void (*)(const float *, uint8_t *, SurfGeom, YuvEncode, Dither, int64_t);
// [format][chroma]; 4:4:4 has no filter: one kernel for both values
#define BSVD_FMT_ROW(K, F) {K<F, 0>, K<F, 1>}
#define BSVD_FMT_ROW444(K, F) {K<F, 0>, K<F, 0>}
static const DecodeKernel kDecode[N_FORMATS][2] = {
    BSVD_FMT_ROW(yuv_to_planar_kernel, F420P), BSVD_FMT_ROW(yuv_to_planar_kernel, F420P10), BSVD_FMT_ROW(yuv_to_planar_kernel, FUYVY),
    BSVD_FMT_ROW(yuv_to_planar_kernel, FYUYV), BSVD_FMT_ROW(yuv_to_planar_kernel, FNV16), BSVD_FMT_ROW(yuv_to_planar_kernel, FP210),
    BSVD_FMT_ROW(yuv_to_planar_kernel, F422P), BSVD_FMT_ROW(yuv_to_planar_kernel, F422P10), BSVD_FMT_ROW444(yuv_to_planar_kernel, F444P),
    BSVD_FMT_ROW444(yuv_to_planar_kernel, F444P10), BSVD_FMT_ROW(yuv_to_planar_kernel, FNV12), BSVD_FMT_ROW(yuv_to_planar_kernel, FP010)};
static const EncodeKernel kEncode[N_FORMATS][2] = {
    BSVD_FMT_ROW(planar_to_yuv_kernel, F420P), BSVD_FMT_ROW(planar_to_yuv_kernel, F420P10), BSVD_FMT_ROW(planar_to_yuv_kernel, FUYVY),
    BSVD_FMT_ROW(planar_to_yuv_kernel, FYUYV), BSVD_FMT_ROW(planar_to_yuv_kernel, FNV16), BSVD_FMT_ROW(planar_to_yuv_kernel, FP210),
    BSVD_FMT_ROW(planar_to_yuv_kernel, F422P), BSVD_FMT_ROW(planar_to_yuv_kernel, F422P10), BSVD_FMT_ROW444(planar_to_yuv_kernel, F444P),
    BSVD_FMT_ROW444(planar_to_yuv_kernel, F444P10), BSVD_FMT_ROW(planar_to_yuv_kernel, FNV12), BSVD_FMT_ROW(planar_to_yuv_kernel, FP010)};

// what a front's checks leave for the launch: the kernel (fmt, chroma), its geometry and item count, and what the constants are made of
struct SurfPlan { SurfGeom g; int fmt, chroma, bits, matrix, full_range; int64_t items, frame_bytes; };

static const double kMatrix[3][2] = {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}};   // (Kr, Kb): BT.601, BT.709, BT.2020 ncl

static YuvDecode decode_constants(int bits, int matrix, int full_range)
{
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kMatrix[matrix][0], kb = kMatrix[matrix][1], kg = 1.0 - kr - kb;
    YuvDecode k;
    k.y_off = full_range ? 0.f : (float)(16 * s);
    k.y_mul = (float)(1.0 / (full_range ? top : 219 * s));
    k.c_off = full_range ? (float)(1 << (bits - 1)) : (float)(128 * s);
    k.c_mul = (float)(1.0 / (full_range ? top : 224 * s));
    k.r_cr = (float)(2 * (1 - kr));
    k.g_cr = (float)(2 * kr * (1 - kr) / kg);
    k.g_cb = (float)(2 * kb * (1 - kb) / kg);
    k.b_cb = (float)(2 * (1 - kb));
    return k;
}

static YuvEncode encode_constants(int bits, int matrix, int full_range)
{
    const double s = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double kr = kMatrix[matrix][0], kb = kMatrix[matrix][1], kg = 1.0 - kr - kb;
    const double cs = full_range ? top : 224 * s;
    YuvEncode k;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
    k.y_mul = (float)(full_range ? top : 219 * s);
    k.y_off = full_range ? 0.f : (float)(16 * s);
    k.cb_mul = (float)(cs / (2 * (1 - kb)));
    k.cr_mul = (float)(cs / (2 * (1 - kr)));
    k.c_off = full_range ? (float)(1 << (bits - 1)) : (float)(128 * s);
    k.y_lo = k.c_lo = full_range ? 0.f : (float)(16 * s);
    k.y_hi = full_range ? (float)top : (float)(235 * s);
    k.c_hi = full_range ? (float)top : (float)(240 * s);
    return k;
}

// One call of an entry point as the checks see it: the function's name, the surface and the tensor with the names their parameters have in
// it (src / dst), the picture H x W, and for the pad / crop entry points (pad != 0) the tensor Hp x Wp.
struct YuvCall { const char *fn; const void *yuv; const char *yuv_name; const float *planar; const char *planar_name; int32_t frames, H, W; int pad; int32_t Hp, Wp; };

// The checks the two fronts make in the same words.  First: the pointers (`desc`: the front's description, "desc" or "surface"), the
// frame count and the sizes of the plain entry points, H and W multiples of 4.
static int args_check(const YuvCall &c, const void *desc, const char *desc_name)
{
    if (!c.yuv) { set_error("%s: %s is NULL", c.fn, c.yuv_name); return -3; }
    if (!c.planar) { set_error("%s: %s is NULL", c.fn, c.planar_name); return -3; }
    if (!desc) { set_error("%s: %s is NULL", c.fn, desc_name); return -3; }
    if (c.frames <= 0) { set_error("%s: frames = %d must be positive", c.fn, c.frames); return -3; }
    if (!c.pad) {
        if (c.H <= 0 || (c.H & 3)) { set_error("%s: H = %d must be a positive multiple of 4", c.fn, c.H); return -3; }
        if (c.W <= 0 || (c.W & 3)) { set_error("%s: W = %d must be a positive multiple of 4", c.fn, c.W); return -3; }
    }
    return 0;
}

// ... the planar tensor of the pad / crop entry points against the picture.  hp_even: Hp must be even (4:2:0); hp_note: what that message
// adds, the one wording in which the fronts differ
static int pad_check(const YuvCall &c, bool hp_even, const char *hp_note)
{
    const char *fn = c.fn;
    const int32_t H = c.H, W = c.W, Hp = c.Hp, Wp = c.Wp;
    if (Hp < H) { set_error("%s: Hp = %d is below H = %d", fn, Hp, H); return -3; }
    if (Wp < W) { set_error("%s: Wp = %d is below W = %d", fn, Wp, W); return -3; }
    if (Hp - H >= H) { set_error("%s: Hp = %d pads H = %d by a whole dimension or more (reflect is defined up to 2 H - 1)", fn, Hp, H); return -3; }
    if (Wp - W >= W) { set_error("%s: Wp = %d pads W = %d by a whole dimension or more (reflect is defined up to 2 W - 1)", fn, Wp, W); return -3; }
    if (hp_even && (Hp & 1)) { set_error("%s: Hp = %d must be even%s", fn, Hp, hp_note); return -3; }
    if (Wp & 3) { set_error("%s: Wp = %d must be a multiple of 4 (rows move as float4)", fn, Wp); return -3; }
    return 0;
}

// ... and last the tensor's alignment and the item count (item_rows: H, or H / 2 with 4:2:0), which complete the plan
static int plan_check(const YuvCall &c, int item_rows, SurfPlan *p)
{
    if ((uintptr_t)c.planar & 15) { set_error("%s: %s must be 16-byte aligned (rows move as float4)", c.fn, c.planar_name); return -3; }
    const int64_t per_frame = (int64_t)item_rows * items_per_row(c.W);
    if (per_frame > 0x7fffffff) { set_error("%s: H x W = %d x %d: more than 2^31 items per frame", c.fn, c.H, c.W); return -3; }
    p->items = per_frame * c.frames;
    p->g.H = c.H; p->g.W = c.W; p->g.Hp = c.pad ? c.Hp : c.H; p->g.Wp = c.pad ? c.Wp : c.W; p->g.cc = 0; p->g.const_val = 0.f;
    return 0;
}

static int launch_decode(const char *fn, SurfPlan &p, const void *src, float *dst, int32_t const_channels, float const_value, void *stream)
{
    if (const_channels < 0) { set_error("%s: const_channels = %d must not be negative", fn, const_channels); return -3; }
    p.g.cc = const_channels;
    p.g.const_val = const_value;
    return launch_sweep(kDecode[p.fmt][p.chroma], p.items, stream, (const uint8_t *)src, dst, p.g, decode_constants(p.bits, p.matrix, p.full_range), p.items);
}

// dither == NULL: off (the entry points without a BsvdDither).  Checked after the call's other arguments.
static int launch_encode(const char *fn, const SurfPlan &p, const float *src, void *dst, const BsvdDither *dither, void *stream)
{
    Dither di;
    if (dither_check(fn, dither, &di)) return -3;
    return launch_sweep(kEncode[p.fmt][p.chroma], p.items, stream, src, (uint8_t *)dst, p.g, encode_constants(p.bits, p.matrix, p.full_range), di, p.items);
}

// ---------------------------------------------------------------------------------------------
// the BsvdYuvSurface front: bsvd_yuv_*

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
    p->chroma = s->chroma; p->bits = s->bits; p->matrix = s->matrix; p->full_range = s->full_range;

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

static int yuv_surface_check(const YuvCall &c, const BsvdYuvSurface *s, SurfPlan *p)
{
    if (args_check(c, s, "surface")) return -3;
    if (c.pad && (picture_check(c.fn, c.H, c.W, s->subsampling) || pad_check(c, s->subsampling == BSVD_SUB_420, " (4:2:0)"))) return -3;
    const int rc = surface_check(c.fn, c.H, c.W, s, p);
    if (rc) return rc;
    if (s->bits == 10 && ((uintptr_t)c.yuv & 1)) { set_error("%s: %s must be 2-byte aligned with 16-bit samples", c.fn, c.yuv_name); return -3; }
    return plan_check(c, s->subsampling == BSVD_SUB_420 ? c.H / 2 : c.H, p);
}

static int decode(const char *fn, const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                  const BsvdYuvSurface *s, int32_t const_channels, float const_value, void *stream)
{
    SurfPlan p;
    const int rc = yuv_surface_check({fn, src, "src", dst, "dst", frames, H, W, pad, Hp, Wp}, s, &p);
    return rc ? rc : launch_decode(fn, p, src, dst, const_channels, const_value, stream);
}

static int encode(const char *fn, const float *src, void *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                  const BsvdYuvSurface *s, const BsvdDither *dither, void *stream)
{
    SurfPlan p;
    const int rc = yuv_surface_check({fn, dst, "dst", src, "src", frames, H, W, pad, Hp, Wp}, s, &p);
    return rc ? rc : launch_encode(fn, p, src, dst, dither, stream);
}

// ---------------------------------------------------------------------------------------------
// the BsvdYuvDesc front: bsvd_yuv420_*.  NV12 / P010 are the semi-planar 4:2:0 rows of the tables with one pitch for both planes and the
// CbCr plane directly behind the H rows of Y.
static inline int sample_bytes(int pix_fmt) { return pix_fmt == BSVD_PIX_P010 ? 2 : 1; }

// the pad / crop entry points take H and W even
static int yuv420_check(const YuvCall &c, const BsvdYuvDesc *d, SurfPlan *p)
{
    const char *fn = c.fn;
    const int32_t H = c.H, W = c.W;
    if (args_check(c, d, "desc")) return -3;
    if (c.pad) {
        if (H <= 0 || (H & 1)) { set_error("%s: H = %d must be positive and even (4:2:0)", fn, H); return -3; }
        if (W <= 0 || (W & 1)) { set_error("%s: W = %d must be positive and even (4:2:0)", fn, W); return -3; }
        if (pad_check(c, true, "")) return -3;
    }
    if (d->pix_fmt != BSVD_PIX_NV12 && d->pix_fmt != BSVD_PIX_P010) { set_error("%s: desc->pix_fmt = %d (BSVD_PIX_NV12, BSVD_PIX_P010)", fn, d->pix_fmt); return -3; }
    if (d->matrix < BSVD_MATRIX_BT601 || d->matrix > BSVD_MATRIX_BT2020) { set_error("%s: desc->matrix = %d (BSVD_MATRIX_BT601 .. BT2020)", fn, d->matrix); return -3; }
    if (d->full_range != 0 && d->full_range != 1) { set_error("%s: desc->full_range = %d (0 or 1)", fn, d->full_range); return -3; }
    if (d->chroma != BSVD_CHROMA_NEAREST && d->chroma != BSVD_CHROMA_LINEAR) { set_error("%s: desc->chroma = %d (BSVD_CHROMA_NEAREST, BSVD_CHROMA_LINEAR)", fn, d->chroma); return -3; }
    if (d->reserved != 0) { set_error("%s: desc->reserved = %d must be 0", fn, d->reserved); return -3; }
    const int sb = sample_bytes(d->pix_fmt);
    const int64_t tight = (int64_t)W * sb;
    const int64_t pitch = d->row_pitch ? d->row_pitch : tight;
    if (pitch < tight) { set_error("%s: desc->row_pitch = %d bytes is below W = %d samples (%lld bytes)", fn, d->row_pitch, W, (long long)tight); return -3; }
    const int64_t frame = pitch * H / 2 * 3;
    const int64_t fstride = d->frame_stride ? d->frame_stride : frame;
    if (fstride < frame) { set_error("%s: desc->frame_stride = %lld bytes is below one frame (%lld bytes)", fn, (long long)d->frame_stride, (long long)frame); return -3; }
    if (sb == 2) {
        if (pitch & 1) { set_error("%s: desc->row_pitch = %d must be a multiple of 2 with BSVD_PIX_P010", fn, d->row_pitch); return -3; }
        if (fstride & 1) { set_error("%s: desc->frame_stride = %lld must be a multiple of 2 with BSVD_PIX_P010", fn, (long long)d->frame_stride); return -3; }
        if ((uintptr_t)c.yuv & 1) { set_error("%s: %s must be 2-byte aligned with BSVD_PIX_P010", fn, c.yuv_name); return -3; }
    }
    p->fmt = FMT_NV12 + d->pix_fmt;
    p->chroma = d->chroma; p->bits = sb == 2 ? 10 : 8; p->matrix = d->matrix; p->full_range = d->full_range;
    p->g.fstride = fstride;
    p->g.off[0] = 0; p->g.off[1] = H * pitch; p->g.off[2] = 0;
    p->g.pitch[0] = p->g.pitch[1] = pitch; p->g.pitch[2] = 0;
    return plan_check(c, H / 2, p);
}

static int64_t yuv_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch, int mask)
{
    if (H <= 0 || W <= 0 || (H & mask) || (W & mask) || (pix_fmt != BSVD_PIX_NV12 && pix_fmt != BSVD_PIX_P010) || row_pitch < 0) return -1;
    const int sb = sample_bytes(pix_fmt);
    const int64_t pitch = row_pitch ? row_pitch : (int64_t)W * sb;
    if (pitch < (int64_t)W * sb || (pitch & (sb - 1))) return -1;
    return pitch * H / 2 * 3;
}

static int decode420(const char *fn, const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                     const BsvdYuvDesc *d, int32_t const_channels, float const_value, void *stream)
{
    SurfPlan p;
    const int rc = yuv420_check({fn, src, "src", dst, "dst", frames, H, W, pad, Hp, Wp}, d, &p);
    return rc ? rc : launch_decode(fn, p, src, dst, const_channels, const_value, stream);
}

static int encode420(const char *fn, const float *src, void *dst, int32_t frames, int32_t H, int32_t W, int pad, int32_t Hp, int32_t Wp,
                     const BsvdYuvDesc *d, const BsvdDither *dither, void *stream)
{
    SurfPlan p;
    const int rc = yuv420_check({fn, dst, "dst", src, "src", frames, H, W, pad, Hp, Wp}, d, &p);
    return rc ? rc : launch_encode(fn, p, src, dst, dither, stream);
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
    return encode("bsvd_planar_to_yuv", src, dst, frames, H, W, 0, 0, 0, surface, nullptr, stream);
}

int bsvd_yuv_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const BsvdYuvSurface *surface,
                           int32_t const_channels, float const_value, void *stream)
{
    return decode("bsvd_yuv_to_planar_pad", src, dst, frames, H, W, 1, Hp, Wp, surface, const_channels, const_value, stream);
}

int bsvd_planar_to_yuv_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvSurface *surface,
                            void *stream)
{
    return encode("bsvd_planar_to_yuv_crop", src, dst, frames, H, W, 1, Hp, Wp, surface, nullptr, stream);
}

int bsvd_planar_to_yuv_crop_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvSurface *surface,
                              const BsvdDither *dither, void *stream)
{
    if (!dither) { set_error("bsvd_planar_to_yuv_crop_d: dither is NULL"); return -3; }
    return encode("bsvd_planar_to_yuv_crop_d", src, dst, frames, H, W, 1, Hp, Wp, surface, dither, stream);
}

int64_t bsvd_yuv420_frame_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch) { return yuv_bytes(H, W, pix_fmt, row_pitch, 3); }
int64_t bsvd_yuv420_picture_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch) { return yuv_bytes(H, W, pix_fmt, row_pitch, 1); }

int bsvd_yuv420_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc, int32_t const_channels,
                          float const_value, void *stream)
{
    return decode420("bsvd_yuv420_to_planar", src, dst, frames, H, W, 0, 0, 0, desc, const_channels, const_value, stream);
}

int bsvd_planar_to_yuv420(const float *src, void *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc, void *stream)
{
    return encode420("bsvd_planar_to_yuv420", src, dst, frames, H, W, 0, 0, 0, desc, nullptr, stream);
}

int bsvd_yuv420_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const BsvdYuvDesc *desc,
                              int32_t const_channels, float const_value, void *stream)
{
    return decode420("bsvd_yuv420_to_planar_pad", src, dst, frames, H, W, 1, Hp, Wp, desc, const_channels, const_value, stream);
}

int bsvd_planar_to_yuv420_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvDesc *desc,
                               void *stream)
{
    return encode420("bsvd_planar_to_yuv420_crop", src, dst, frames, H, W, 1, Hp, Wp, desc, nullptr, stream);
}

int bsvd_planar_to_yuv420_crop_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdYuvDesc *desc,
                                 const BsvdDither *dither, void *stream)
{
    if (!dither) { set_error("bsvd_planar_to_yuv420_crop_d: dither is NULL"); return -3; }
    return encode420("bsvd_planar_to_yuv420_crop_d", src, dst, frames, H, W, 1, Hp, Wp, desc, dither, stream);
}

}  // extern "C"
