// frame_rgb.hip -- RGB surfaces on the device (include/bsvd_hip.h, BsvdRgbSurface): packed pixels of 3 or 4 samples in any order, 8 to 16
// bit, 2:10:10:10 words and planar GBR(A) <-> the planar fp32 tensors of the network, with reflect pad / crop in the kernel and alpha
// carried beside the tensor as a plane of codes.  The RGB counterpart of frame_yuv.hip: helper kernels on the caller's stream, outside the
// captured graphs, bandwidth-bound, grid-stride loops around the item bodies of frame_rgb_items.h.  Nine instantiations per direction
// ({packed, planar} x {1-byte, 2-byte samples} x {3, 4 slots}, and the x2 word) serve every name: component order, sample mask and scale
// are kernel arguments.  Compiled without contraction (sources.sh): the header states the arithmetic operation by operation.
#include "bsvd_internal.h"
#include "frame_rgb_items.h"

namespace bsvd {

template <class F>
__global__ __launch_bounds__(256) void rgb_to_planar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, void *__restrict__ alpha, RgbGeom g, RgbDecode k, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        rgb_to_planar_item<F>(src, dst, alpha, g, k, i);
}

template <class F>
__global__ __launch_bounds__(256) void planar_to_rgb_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, const void *__restrict__ alpha, RgbGeom g, RgbEncode k, Dither di, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        planar_to_rgb_item<F>(src, dst, alpha, g, k, di, i);
}

// ---------------------------------------------------------------------------------------------
// host side: the table, validation (no device needed), constants, dispatch
using DecodeKernel = void (*)(const uint8_t *, float *, void *, RgbGeom, RgbDecode, int64_t);
using EncodeKernel = void (*)(const float *, uint8_t *, const void *, RgbGeom, RgbEncode, Dither, int64_t);
// [packed 0 | planar 1][sample bytes - 1][slots - 3], then the x2 word
#define BSVD_RGB_TABLE(K) {{{K<RgbFmt<BSVD_RGB_PACKED, 1, 3>>, K<RgbFmt<BSVD_RGB_PACKED, 1, 4>>}, {K<RgbFmt<BSVD_RGB_PACKED, 2, 3>>, K<RgbFmt<BSVD_RGB_PACKED, 2, 4>>}}, \
                           {{K<RgbFmt<BSVD_RGB_PLANAR, 1, 3>>, K<RgbFmt<BSVD_RGB_PLANAR, 1, 4>>}, {K<RgbFmt<BSVD_RGB_PLANAR, 2, 3>>, K<RgbFmt<BSVD_RGB_PLANAR, 2, 4>>}}}
static const DecodeKernel kDecode[2][2][2] = BSVD_RGB_TABLE(rgb_to_planar_kernel);
static const EncodeKernel kEncode[2][2][2] = BSVD_RGB_TABLE(planar_to_rgb_kernel);
static const DecodeKernel kDecodeX2 = rgb_to_planar_kernel<RgbFmt<BSVD_RGB_PACKED_X2_10, 4, 3>>;
static const EncodeKernel kEncodeX2 = planar_to_rgb_kernel<RgbFmt<BSVD_RGB_PACKED_X2_10, 4, 3>>;

struct RgbPlan { RgbGeom g; int align, bits, full_range; int64_t frame_bytes; };

// The surface's own description: enums, counts, positions, pitches, offsets, stride.  H x W (positive) is the surface's picture.
static int surface_check(const char *fn, int32_t H, int32_t W, const BsvdRgbSurface *s, RgbPlan *p)
{
    if (s->layout < BSVD_RGB_PACKED || s->layout > BSVD_RGB_PLANAR) { set_error("%s: surface->layout = %d (BSVD_RGB_PACKED .. BSVD_RGB_PLANAR)", fn, s->layout); return -3; }
    const bool x2 = s->layout == BSVD_RGB_PACKED_X2_10;
    if (s->components != 3 && s->components != 4) { set_error("%s: surface->components = %d (3 or 4)", fn, s->components); return -3; }
    if (x2 && s->components != 3) { set_error("%s: surface->components = %d (3 with BSVD_RGB_PACKED_X2_10)", fn, s->components); return -3; }
    if (s->bits != 8 && s->bits != 10 && s->bits != 12 && s->bits != 16) { set_error("%s: surface->bits = %d (8, 10, 12 or 16)", fn, s->bits); return -3; }
    if (x2 && s->bits != 10) { set_error("%s: surface->bits = %d: BSVD_RGB_PACKED_X2_10 carries 10 bits", fn, s->bits); return -3; }
    if (s->fourth < BSVD_RGB_FOURTH_NONE || s->fourth > BSVD_RGB_FOURTH_FILLER) { set_error("%s: surface->fourth = %d (BSVD_RGB_FOURTH_NONE .. FILLER)", fn, s->fourth); return -3; }
    if ((s->components == 4) != (s->fourth != BSVD_RGB_FOURTH_NONE)) { set_error("%s: surface->fourth = %d with components = %d (a fourth sample is alpha or a filler; three have none)", fn, s->fourth, s->components); return -3; }
    if (s->full_range != 0 && s->full_range != 1) { set_error("%s: surface->full_range = %d (0 or 1)", fn, s->full_range); return -3; }
    if (s->reserved0 != 0) { set_error("%s: surface->reserved0 = %d must be 0", fn, s->reserved0); return -3; }
    if (s->reserved != 0) { set_error("%s: surface->reserved = %lld must be 0", fn, (long long)s->reserved); return -3; }
    RgbGeom &g = p->g;
    for (int j = 0; j < 4; ++j) g.chan[j] = -1;
    for (int c = 0; c < 4; ++c) {
        const int at = s->pos[c];
        if (c >= s->components) {
            if (at != 0) { set_error("%s: surface->pos[%d] = %d must be 0 with %d components", fn, c, at, s->components); return -3; }
            continue;
        }
        if (at < 0 || at >= s->components || g.chan[at] >= 0) { set_error("%s: surface->pos[%d] = %d: pos is no permutation of 0 .. %d", fn, c, at, s->components - 1); return -3; }
        g.chan[at] = c;
    }
    if (s->components == 3) g.chan[3] = 3;
    p->bits = s->bits; p->full_range = s->full_range;
    g.mask = (1u << s->bits) - 1;

    const int sb = s->bits == 8 ? 1 : 2;
    const int planes = s->layout == BSVD_RGB_PLANAR ? s->components : 1;
    const int64_t row_bytes = x2 ? (int64_t)W * 4 : (int64_t)W * sb * (planes == 1 ? s->components : 1);
    p->align = x2 ? 4 : sb;
    int64_t end = 0;
    for (int i = 0; i < 4; ++i) {
        if (i >= planes) {
            if (s->pitch[i] != 0) { set_error("%s: surface->pitch[%d] = %d must be 0: the layout has %d plane(s)", fn, i, s->pitch[i], planes); return -3; }
            if (s->offset[i] != 0) { set_error("%s: surface->offset[%d] = %lld must be 0: the layout has %d plane(s)", fn, i, (long long)s->offset[i], planes); return -3; }
            g.pitch[i] = g.off[i] = 0;
            continue;
        }
        g.pitch[i] = s->pitch[i] ? s->pitch[i] : row_bytes;
        if (g.pitch[i] < row_bytes) { set_error("%s: surface->pitch[%d] = %d bytes is below the plane's row (%lld bytes)", fn, i, s->pitch[i], (long long)row_bytes); return -3; }
        if (s->offset[i] < 0) { set_error("%s: surface->offset[%d] = %lld must not be negative", fn, i, (long long)s->offset[i]); return -3; }
        g.off[i] = i == 0 || s->offset[i] ? s->offset[i] : g.off[i - 1] + g.pitch[i - 1] * H;
        if (g.pitch[i] & (p->align - 1)) { set_error("%s: surface->pitch[%d] = %d must be a multiple of %d (the sample's alignment)", fn, i, s->pitch[i], p->align); return -3; }
        if (g.off[i] & (p->align - 1)) { set_error("%s: surface->offset[%d] = %lld must be a multiple of %d (the sample's alignment)", fn, i, (long long)s->offset[i], p->align); return -3; }
        for (int k = 0; k < i; ++k)
            if (g.off[i] < g.off[k] + g.pitch[k] * H && g.off[k] < g.off[i] + g.pitch[i] * H) {
                set_error("%s: surface->offset[%d] = %lld: planes %d and %d share bytes", fn, i, (long long)s->offset[i], k, i);
                return -3;
            }
        const int64_t e = g.off[i] + g.pitch[i] * H;
        if (e > end) end = e;
    }
    p->frame_bytes = end;
    g.fstride = s->frame_stride ? s->frame_stride : end;
    if (g.fstride < end) { set_error("%s: surface->frame_stride = %lld bytes is below one frame (%lld bytes)", fn, (long long)s->frame_stride, (long long)end); return -3; }
    if (g.fstride & (p->align - 1)) { set_error("%s: surface->frame_stride = %lld must be a multiple of %d (the sample's alignment)", fn, (long long)s->frame_stride, p->align); return -3; }
    return 0;
}

// One call as the checks see it: the surface and the tensor with the names their parameters have (src / dst), the alpha side plane and its name
struct RgbCall { const char *fn; const void *rgb; const char *rgb_name; const float *planar; const char *planar_name; const void *alpha; const char *alpha_name;
                 int32_t frames, H, W, Hp, Wp; };

static int rgb_check(const RgbCall &c, const BsvdRgbSurface *s, RgbPlan *p, int64_t *items)
{
    const char *fn = c.fn;
    if (!c.rgb) { set_error("%s: %s is NULL", fn, c.rgb_name); return -3; }
    if (!c.planar) { set_error("%s: %s is NULL", fn, c.planar_name); return -3; }
    if (!s) { set_error("%s: surface is NULL", fn); return -3; }
    if (c.frames <= 0) { set_error("%s: frames = %d must be positive", fn, c.frames); return -3; }
    if (c.H <= 0) { set_error("%s: H = %d must be positive", fn, c.H); return -3; }
    if (c.W <= 0) { set_error("%s: W = %d must be positive", fn, c.W); return -3; }
    if (c.Hp < c.H) { set_error("%s: Hp = %d is below H = %d", fn, c.Hp, c.H); return -3; }
    if (c.Wp < c.W) { set_error("%s: Wp = %d is below W = %d", fn, c.Wp, c.W); return -3; }
    if (c.Hp - c.H >= c.H) { set_error("%s: Hp = %d pads H = %d by a whole dimension or more (reflect is defined up to 2 H - 1)", fn, c.Hp, c.H); return -3; }
    if (c.Wp - c.W >= c.W) { set_error("%s: Wp = %d pads W = %d by a whole dimension or more (reflect is defined up to 2 W - 1)", fn, c.Wp, c.W); return -3; }
    const int rc = surface_check(fn, c.H, c.W, s, p);
    if (rc) return rc;
    if ((uintptr_t)c.rgb & (p->align - 1)) { set_error("%s: %s must be %d-byte aligned (the sample's alignment)", fn, c.rgb_name, p->align); return -3; }
    if ((uintptr_t)c.planar & 3) { set_error("%s: %s must be 4-byte aligned", fn, c.planar_name); return -3; }
    if (c.alpha) {
        if (s->fourth != BSVD_RGB_FOURTH_ALPHA) { set_error("%s: %s given for a surface without alpha (surface->fourth = %d)", fn, c.alpha_name, s->fourth); return -3; }
        if ((uintptr_t)c.alpha & (p->align - 1)) { set_error("%s: %s must be %d-byte aligned (the sample's alignment)", fn, c.alpha_name, p->align); return -3; }
    }
    const int64_t per_frame = (int64_t)c.H * items_per_row(c.W);
    if (per_frame > 0x7fffffff) { set_error("%s: H x W = %d x %d: more than 2^31 items per frame", fn, c.H, c.W); return -3; }
    *items = per_frame * c.frames;
    RgbGeom &g = p->g;
    g.H = c.H; g.W = c.W; g.Hp = c.Hp; g.Wp = c.Wp; g.cc = 0; g.const_val = 0.f;
    g.vec = (c.Wp & 3) == 0 && aligned16(c.planar);
    return 0;
}

// first index of the kernel tables: packed 0, planar 1 (the x2 word has its own pair)
static inline int table_row(const BsvdRgbSurface *s) { return s->layout == BSVD_RGB_PLANAR; }

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_rgb_frame_bytes(int32_t H, int32_t W, const BsvdRgbSurface *surface)
{
    RgbPlan p;
    if (!surface || H <= 0 || W <= 0) return -1;
    if (surface_check("bsvd_rgb_frame_bytes", H, W, surface, &p)) return -1;
    return p.frame_bytes;
}

int bsvd_rgb_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, const BsvdRgbSurface *surface,
                       void *alpha_out, int32_t const_channels, float const_value, void *stream)
{
    const char *fn = "bsvd_rgb_to_planar";
    RgbPlan p;
    int64_t items = 0;
    const int rc = rgb_check({fn, src, "src", dst, "dst", alpha_out, "alpha_out", frames, H, W, Hp, Wp}, surface, &p, &items);
    if (rc) return rc;
    if (const_channels < 0) { set_error("%s: const_channels = %d must not be negative", fn, const_channels); return -3; }
    p.g.cc = const_channels;
    p.g.const_val = const_value;
    const float s = (float)(1 << (p.bits - 8));
    RgbDecode k;
    k.sub = p.full_range ? 0.f : 16.f * s;
    k.div = p.full_range ? (float)((1u << p.bits) - 1) : 219.f * s;
    const DecodeKernel kern = surface->layout == BSVD_RGB_PACKED_X2_10 ? kDecodeX2 : kDecode[table_row(surface)][p.bits > 8][surface->components - 3];
    return launch_sweep(kern, items, stream, (const uint8_t *)src, dst, alpha_out, p.g, k, items);
}

// dither == NULL: off (bsvd_planar_to_rgb)
static int encode_rgb(const char *fn, const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdRgbSurface *surface,
                      const void *alpha_in, const BsvdDither *dither, void *stream)
{
    RgbPlan p;
    int64_t items = 0;
    const int rc = rgb_check({fn, dst, "dst", src, "src", alpha_in, "alpha_in", frames, H, W, Hp, Wp}, surface, &p, &items);
    if (rc) return rc;
    Dither di;
    if (dither_check(fn, dither, &di)) return -3;
    const float s = (float)(1 << (p.bits - 8)), top = (float)((1u << p.bits) - 1);
    RgbEncode k;
    k.mul = p.full_range ? top : 219.f * s;
    k.add = p.full_range ? 0.f : 16.f * s;
    k.lo = k.add;
    k.hi = p.full_range ? top : 235.f * s;
    k.fill = p.g.mask;
    const EncodeKernel kern = surface->layout == BSVD_RGB_PACKED_X2_10 ? kEncodeX2 : kEncode[table_row(surface)][p.bits > 8][surface->components - 3];
    return launch_sweep(kern, items, stream, src, (uint8_t *)dst, alpha_in, p.g, k, di, items);
}

int bsvd_planar_to_rgb(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdRgbSurface *surface,
                       const void *alpha_in, void *stream)
{
    return encode_rgb("bsvd_planar_to_rgb", src, dst, frames, Hp, Wp, H, W, surface, alpha_in, nullptr, stream);
}

int bsvd_planar_to_rgb_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W, const BsvdRgbSurface *surface,
                         const void *alpha_in, const BsvdDither *dither, void *stream)
{
    if (!dither) { set_error("bsvd_planar_to_rgb_d: dither is NULL"); return -3; }
    return encode_rgb("bsvd_planar_to_rgb_d", src, dst, frames, Hp, Wp, H, W, surface, alpha_in, dither, stream);
}

}  // extern "C"
