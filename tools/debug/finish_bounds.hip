// finish_bounds.hip -- runs the item bodies of the output finish (bsvd_amd/csrc/frame_finish_items.h: the blend; frame_surface_items.h and
// frame_rgb_items.h: the encoders with both dithers) on the HOST, over heap buffers of exactly the bytes the ABI promises, under
// AddressSanitizer and UBSan, in the manner of yuv_surface_bounds.hip / rgb_surface_bounds.hip: the slack between the blend's frames, the
// bytes around the fp32 tensors and every byte of a surface that is no sample are outside the allocation or poisoned, so a read or write
// there stops the program.  Pictures end their rows in part items (W % 4 in 1 .. 3 for RGB and 4:4:4, W % 4 == 2 for subsampled chroma),
// pitches carry an odd slack, and Hp > H, Wp > W.  It also checks what needs no model: the blend's exact ends and the float4 side against
// the scalar side; dither off equal to the bodies' old form; NaN in the pad region reaching no sample; bytes that are no sample untouched;
// and the whole-code property of the RGB encoder -- a tensor of exact codes comes back as those codes under both dithers, at 8 to 16 bits.
// Host code only: no kernel is launched and no device is needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/finish_bounds.hip -o build/finish_bounds && build/finish_bounds
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_surface_items.h"
#include "frame_rgb_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// n floats of exactly their bytes, `lead` floats behind a 16-byte boundary; values in [-0.25, 1.25)
struct Floats { char *base; float *p; int64_t n; };
static Floats alloc_floats(int64_t n, int lead)
{
    const size_t bytes = (size_t)(((n + lead) * 4 + 15) / 16 * 16);
    Floats a;
    a.base = (char *)aligned_alloc(16, bytes);
    a.p = (float *)a.base + lead;
    a.n = n;
    for (int64_t i = 0; i < n; ++i) a.p[i] = (float)(rnd() & 0xffff) / 65536.f * 1.5f - 0.25f;
    if (lead) __asan_poison_memory_region(a.base, lead * 4);
    if (bytes > (size_t)(n + lead) * 4) __asan_poison_memory_region((char *)(a.p + n), bytes - (size_t)(n + lead) * 4);
    return a;
}
static void release(Floats &a) { free(a.base); }

// ---------------------------------------------------------------------------------------------
// the blend: y frames 3 planes + slack apart, x frames 4 planes apart; the slack and the fourth plane of x are poisoned
static void blend_case(int T, int Hp, int Wp, int slack, int lead, float s_l, float s_c)
{
    const int64_t plane = (int64_t)Hp * Wp, y_fs = 3 * plane + slack, x_fs = 4 * plane;
    Floats y = alloc_floats((T - 1) * y_fs + 3 * plane, lead), x = alloc_floats((T - 1) * x_fs + 3 * plane, lead);
    std::vector<float> y0(y.p, y.p + y.n), x0(x.p, x.p + x.n);
    for (int f = 0; f + 1 < T; ++f) {
        if (slack) __asan_poison_memory_region(y.p + f * y_fs + 3 * plane, slack * 4);
        __asan_poison_memory_region(x.p + f * x_fs + 3 * plane, plane * 4);
    }
    BlendGeom g;
    g.y_fs = y_fs; g.x_fs = x_fs; g.plane = plane;
    g.vec = (Wp & 3) == 0 && lead == 0 && (y_fs & 3) == 0;
    g.per_frame = g.vec ? plane / 4 : plane;
    g.s_c = s_c; g.om = (float)(1.0 - (double)s_c); g.dl = s_c - s_l;
    g.w[0] = 0.2126f; g.w[1] = 0.7152f; g.w[2] = 0.0722f;
    for (int64_t i = 0; i < g.per_frame * T; ++i) blend_planar_item(y.p, x.p, g, i);
    // the scalar path on copies: the same bits
    std::vector<float> ys(y0);
    BlendGeom gs = g;
    gs.vec = 0; gs.per_frame = plane;
    for (int64_t i = 0; i < plane * T; ++i) blend_planar_item(ys.data(), x0.data(), gs, i);
    for (int f = 0; f < T; ++f)
        for (int64_t e = 0; e < 3 * plane; ++e) {
            const int64_t iy = f * y_fs + e, ix = f * x_fs + e;
            EXPECT(memcmp(&y.p[iy], &ys[iy], 4) == 0, "blend %dx%d vec%d: the float4 side differs from the scalar side at %lld", Hp, Wp, g.vec, (long long)iy);
            if (s_l == 1.f && s_c == 1.f) EXPECT(memcmp(&y.p[iy], &y0[iy], 4) == 0, "blend (1,1) is not y at %lld", (long long)iy);
            if (s_l == 0.f && s_c == 0.f) EXPECT(memcmp(&y.p[iy], &x0[ix], 4) == 0, "blend (0,0) is not x at %lld", (long long)iy);
            if (s_l == s_c) { const float m = s_c * y0[iy] + g.om * x0[ix]; EXPECT(memcmp(&y.p[iy], &m, 4) == 0, "blend (s,s) is not the lerp at %lld", (long long)iy); }
        }
    for (int f = 0; f + 1 < T; ++f) {
        if (slack) __asan_unpoison_memory_region(y.p + f * y_fs + 3 * plane, slack * 4);
        __asan_unpoison_memory_region(x.p + f * x_fs + 3 * plane, plane * 4);
        for (int q = 0; q < slack; ++q) EXPECT(memcmp(&y.p[f * y_fs + 3 * plane + q], &y0[f * y_fs + 3 * plane + q], 4) == 0, "blend wrote into the slack");
    }
    release(y); release(x);
}

// ---------------------------------------------------------------------------------------------
// surfaces of exactly their bytes, every byte that is no sample poisoned
struct Surface { uint8_t *p; int64_t bytes; std::vector<uint8_t> is_sample; };
static Surface surface(int T, int planes, const int64_t *rows, const int64_t *row_bytes, const int64_t *off, const int64_t *pitch, int64_t fstride)
{
    Surface s;
    int64_t end = 0;
    for (int i = 0; i < planes; ++i) { const int64_t e = off[i] + pitch[i] * (rows[i] - 1) + row_bytes[i]; if (e > end) end = e; }
    s.bytes = (int64_t)(T - 1) * fstride + end;
    s.p = (uint8_t *)malloc(s.bytes);
    s.is_sample.assign(s.bytes, 0);
    memset(s.p, 0xA5, s.bytes);
    __asan_poison_memory_region(s.p, s.bytes);
    for (int f = 0; f < T; ++f)
        for (int i = 0; i < planes; ++i)
            for (int64_t r = 0; r < rows[i]; ++r) {
                const int64_t at = f * fstride + off[i] + r * pitch[i];
                __asan_unpoison_memory_region(s.p + at, row_bytes[i]);
                memset(s.is_sample.data() + at, 1, row_bytes[i]);
            }
    return s;
}
static void release(Surface &s) { __asan_unpoison_memory_region(s.p, s.bytes); free(s.p); }
// after the runs: the sample bytes of two surfaces compared, the others still 0xA5
static void compare(Surface &a, Surface &b, bool want_equal, const char *what, const char *name)
{
    __asan_unpoison_memory_region(a.p, a.bytes);
    __asan_unpoison_memory_region(b.p, b.bytes);
    int64_t differ = 0, touched = 0;
    for (int64_t i = 0; i < a.bytes; ++i) {
        if (a.is_sample[i]) differ += a.p[i] != b.p[i];
        else touched += a.p[i] != 0xA5 || b.p[i] != 0xA5;
    }
    EXPECT(touched == 0, "%s %s: %lld bytes that are no sample were written", name, what, (long long)touched);
    if (want_equal) EXPECT(differ == 0, "%s %s: %lld sample bytes differ", name, what, (long long)differ);
    else EXPECT(differ > 0, "%s %s: the dither changed no byte", name, what);
}
static void nan_pad(Floats &y, int T, int H, int W, int Hp, int Wp)
{
    const int64_t plane = (int64_t)Hp * Wp;
    for (int64_t f = 0; f < (int64_t)T * 3; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x)
                if (r >= H || x >= W) { const uint32_t u = 0x7fc00000u; memcpy(y.p + f * plane + (int64_t)r * Wp + x, &u, 4); }
}

static const Dither kOff = {BSVD_DITHER_NONE, 0u, 0}, kOrdered = {BSVD_DITHER_ORDERED, 0u, 0}, kRandom = {BSVD_DITHER_RANDOM, 0x5eed1234u, ((int64_t)1 << 33) + 5};

// ---- RGB ----
template <class F>
static void rgb_case(const char *name, int bits, int H, int W, int Hp, int Wp, int lead)
{
    const int T = 2, planes = F::LAY == BSVD_RGB_PLANAR ? F::SLOTS : 1;
    const int64_t plane = (int64_t)Hp * Wp, items = (int64_t)T * H * items_per_row(W);
    const int64_t rb = F::LAY == BSVD_RGB_PLANAR ? (int64_t)W * F::SB : F::LAY == BSVD_RGB_PACKED ? (int64_t)W * F::SB * F::SLOTS : (int64_t)W * 4;
    const int align = F::LAY == BSVD_RGB_PACKED_X2_10 ? 4 : F::SB;
    RgbGeom g = {};
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.vec = (Wp & 3) == 0 && lead == 0;
    for (int j = 0; j < 4; ++j) g.chan[j] = j < F::SLOTS ? (j + 1) % F::SLOTS : 3;
    g.mask = (1u << bits) - 1;
    int64_t rows[4], rbs[4], at = 3 * align;
    for (int i = 0; i < planes; ++i) {
        rows[i] = H; rbs[i] = rb;
        g.pitch[i] = rb + align * (5 + 2 * i);                        // an odd slack, in samples
        g.off[i] = at;
        at += g.pitch[i] * H + 7 * align;
    }
    g.fstride = at + 9 * align;
    const float top = (float)((1u << bits) - 1);
    const RgbEncode ke = {top, 0.f, 0.f, top, g.mask};
    Floats y = alloc_floats((int64_t)T * 3 * plane, lead);
    const Dither modes[3] = {kOff, kOrdered, kRandom};
    Surface plain = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
    for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(y.p, plain.p, nullptr, g, ke, i);
    for (int m = 0; m < 3; ++m) {
        Surface a = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride), b = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
        Floats y2 = alloc_floats((int64_t)T * 3 * plane, lead);
        memcpy(y2.p, y.p, y.n * 4);
        nan_pad(y2, T, H, W, Hp, Wp);
        for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(y.p, a.p, nullptr, g, ke, modes[m], i);
        for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(y2.p, b.p, nullptr, g, ke, modes[m], i);
        compare(a, b, true, m == 0 ? "off, NaN pad" : m == 1 ? "ordered, NaN pad" : "random, NaN pad", name);
        __asan_unpoison_memory_region(plain.p, plain.bytes);
        if (m == 0) EXPECT(memcmp(a.p, plain.p, a.bytes) == 0, "%s: dither off differs from the body's old form", name);
        else compare(a, plain, false, "against dither off", name);
        release(a); release(b); release(y2);
    }
    // whole codes: v = code / top decodes and encodes to itself (bsvd_hip.h); under dither it still does
    Floats w = alloc_floats((int64_t)T * 3 * plane, lead);
    for (int64_t i = 0; i < w.n; ++i) w.p[i] = (float)(rnd() & g.mask) / top;
    Surface ref = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
    for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(w.p, ref.p, nullptr, g, ke, i);
    for (int m = 1; m < 3; ++m) {
        Surface a = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
        for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(w.p, a.p, nullptr, g, ke, modes[m], i);
        compare(a, ref, true, m == 1 ? "whole codes, ordered" : "whole codes, random", name);
        release(a);
    }
    release(ref); release(w); release(plain); release(y);
}

// ---- YUV ----
static const YuvEncode kEnc8 = {0.2126f, 0.7152f, 0.0722f, 219.f, 16.f, 120.7f, 142.2f, 128.f, 16.f, 235.f, 16.f, 240.f};
static const YuvEncode kEnc10 = {0.2126f, 0.7152f, 0.0722f, 876.f, 64.f, 482.9f, 568.9f, 512.f, 64.f, 940.f, 64.f, 960.f};

template <class F, int LINEAR>
static void yuv_case(const char *name, int H, int W, int Hp, int Wp)
{
    const int T = 2;
    const int64_t plane = (int64_t)Hp * Wp, items = (int64_t)T * surf_item_rows<F>(H) * items_per_row(W);
    const int64_t cw = F::SUB == BSVD_SUB_444 ? W : W / 2, ch = F::SUB == BSVD_SUB_420 ? H / 2 : H;
    const int planes = F::PACKED ? 1 : F::LAY == BSVD_LAYOUT_SEMIPLANAR ? 2 : 3;
    const int64_t rows[3] = {H, ch, ch};
    const int64_t rbs[3] = {F::PACKED ? 2 * (int64_t)W : (int64_t)W * F::SB, (F::LAY == BSVD_LAYOUT_SEMIPLANAR ? 2 : 1) * cw * F::SB, cw * F::SB};
    SurfGeom g = {};
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp;
    int64_t at = 3 * F::SB;
    for (int i = 0; i < planes; ++i) {
        g.pitch[i] = rbs[i] + F::SB * (5 + 2 * i);                    // an odd slack, in samples
        g.off[i] = at;
        at += g.pitch[i] * rows[i] + 7 * F::SB;
    }
    g.fstride = at + 9 * F::SB;
    const YuvEncode ke = F::SB == 2 ? kEnc10 : kEnc8;
    Floats y = alloc_floats((int64_t)T * 3 * plane, 0);
    const Dither modes[3] = {kOff, kOrdered, kRandom};
    Surface plain = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
    for (int64_t i = 0; i < items; ++i) planar_to_yuv_item<F, LINEAR>(y.p, plain.p, g, ke, i);
    for (int m = 0; m < 3; ++m) {
        Surface a = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride), b = surface(T, planes, rows, rbs, g.off, g.pitch, g.fstride);
        Floats y2 = alloc_floats((int64_t)T * 3 * plane, 0);
        memcpy(y2.p, y.p, y.n * 4);
        nan_pad(y2, T, H, W, Hp, Wp);
        for (int64_t i = 0; i < items; ++i) planar_to_yuv_item<F, LINEAR>(y.p, a.p, g, ke, modes[m], i);
        for (int64_t i = 0; i < items; ++i) planar_to_yuv_item<F, LINEAR>(y2.p, b.p, g, ke, modes[m], i);
        compare(a, b, true, m == 0 ? "off, NaN pad" : m == 1 ? "ordered, NaN pad" : "random, NaN pad", name);
        __asan_unpoison_memory_region(plain.p, plain.bytes);
        if (m == 0) EXPECT(memcmp(a.p, plain.p, a.bytes) == 0, "%s: dither off differs from the body's old form", name);
        else compare(a, plain, false, "against dither off", name);
        release(a); release(b); release(y2);
    }
    release(plain); release(y);
}

// d itself: the open interval, every Bayer entry once per tile, the extreme hash values
static void d_case()
{
    int seen[64] = {};
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) {
            const unsigned b = bayer8(c, r);
            EXPECT(b < 64, "bayer8(%d,%d) = %u", c, r, b);
            if (b < 64) ++seen[b];
            for (int comp = 0; comp < 3; ++comp) { const float d = dither_ordered(comp, r, c); EXPECT(d > -0.5f && d < 0.5f, "ordered d = %g", (double)d); }
        }
    for (int b = 0; b < 64; ++b) EXPECT(seen[b] == 1, "Bayer entry %d appears %d times", b, seen[b]);
    const unsigned row0[8] = {0, 32, 8, 40, 2, 34, 10, 42};
    for (int c = 0; c < 8; ++c) EXPECT(bayer8(c, 0) == row0[c], "bayer8(%d,0)", c);
    float lo = 1.f, hi = -1.f;
    for (int i = 0; i < 1 << 20; ++i) {
        const float d = dither_random(dither_frame_key(7u, i >> 10, i & 3), i & 1023, i >> 3);
        lo = d < lo ? d : lo; hi = d > hi ? d : hi;
    }
    EXPECT(lo >= -DITHER_RANDOM_MAX && hi <= DITHER_RANDOM_MAX && lo < -0.49f && hi > 0.49f, "random d spans [%g, %g]", (double)lo, (double)hi);
    // rows and columns up to the largest picture, frames beyond 2^32: no undefined arithmetic (UBSan)
    (void)dither_random(dither_frame_key(0xffffffffu, ((int64_t)1 << 62), 2), 0x7ffffffe, 0x7ffffffe);
}

int main()
{
    const float strengths[][2] = {{1.f, 1.f}, {0.f, 0.f}, {0.5f, 0.5f}, {0.3f, 0.9f}, {1.f, 0.f}};
    for (const auto &s : strengths) {
        blend_case(3, 16, 32, 4, 0, s[0], s[1]);      // float4 side
        blend_case(3, 16, 32, 3, 0, s[0], s[1]);      // a stride that is no multiple of 4: scalars
        blend_case(3, 16, 24, 4, 1, s[0], s[1]);      // one float off the 16-byte boundary: scalars
        blend_case(2, 5, 7, 1, 0, s[0], s[1]);        // Wp % 4 != 0
    }
    d_case();
    // RGB: W % 4 = 1, 2, 3 inside larger tensors; the float4 and the scalar fp32 side
    const int rgb_sizes[][4] = {{5, 9, 8, 12}, {10, 22, 16, 24}, {6, 7, 8, 8}, {12, 18, 16, 24}};
    for (const auto &s : rgb_sizes)
        for (int lead = 0; lead < 2; ++lead) {
            rgb_case<RgbFmt<BSVD_RGB_PACKED, 1, 3>>("packed 8 x 3", 8, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PACKED, 1, 4>>("packed 8 x 4", 8, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PACKED, 2, 3>>("packed 16 x 3", 16, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PACKED, 2, 4>>("packed 12 x 4", 12, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PACKED_X2_10, 4, 3>>("x2 10", 10, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PLANAR, 1, 3>>("planar 8 x 3", 8, s[0], s[1], s[2], s[3], lead);
            rgb_case<RgbFmt<BSVD_RGB_PLANAR, 2, 4>>("planar 16 x 4", 16, s[0], s[1], s[2], s[3], lead);
        }
    // YUV: W % 4 == 2 with subsampled chroma, W % 4 = 1 and 3 with 4:4:4
    yuv_case<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_U8>, 1>("yuv420p", 10, 22, 16, 24);
    yuv_case<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_LOW10>, 0>("yuv420p10le", 12, 18, 16, 24);
    yuv_case<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_U8>, 1>("nv12", 10, 22, 16, 24);
    yuv_case<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>, 1>("p010", 6, 10, 8, 12);
    yuv_case<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_UYVY, SMP_U8>, 1>("uyvy422", 5, 10, 8, 12);
    yuv_case<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_YUYV, SMP_U8>, 0>("yuyv422", 5, 22, 8, 24);
    yuv_case<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>, 1>("p210le", 5, 18, 8, 24);
    yuv_case<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_PLANAR, SMP_LOW10>, 1>("yuv422p10le", 7, 6, 8, 8);
    yuv_case<SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_U8>, 0>("yuv444p", 5, 7, 8, 8);
    yuv_case<SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_LOW10>, 0>("yuv444p10le", 6, 9, 8, 12);
    printf("finish_bounds: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
