// yuv_surface_bounds.hip -- runs the item bodies of the YUV kernels (bsvd_amd/csrc/frame_surface_items.h), all twelve formats, on the HOST,
// over heap buffers of exactly the bytes the ABI promises, under AddressSanitizer, in the manner of frame_pad_bounds.hip: every byte of a
// surface that is not a sample -- pitch padding, the bytes between planes and frames, the bytes behind the last sample of the plane that
// ends last -- is outside the allocation or poisoned, so a read or write there stops the program.  nv12 and p010 run with the geometry
// bsvd_yuv420_* gives them (one pitch, CbCr directly behind Y), the ten others with a pitch, an offset and a gap per plane.  It also checks
// what needs no model: every destination element written, pad elements bit-equal to their mirror source, non-sample bytes untouched, NaN
// in the pad region of the fp32 tensor reaching no sample, the ignored bits of 10-bit words reaching no value, and yuv420p / yuv420p10le
// against nv12 / p010 on the same samples, bit for bit.  Host code only: no kernel is launched and no device is needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/yuv_surface_bounds.hip -o build/yuv_surface_bounds && build/yuv_surface_bounds
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_surface_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static const uint32_t UNWRITTEN = 0x7fc12345u;      // a NaN pattern no conversion produces
static int refl(int i, int N) { return i < N ? i : 2 * (N - 1) - i; }

static float *alloc_planes(int64_t n, bool fill_unwritten)
{
    float *p = (float *)aligned_alloc(16, (size_t)((n * 4 + 15) / 16 * 16));
    for (int64_t i = 0; i < n; ++i) { const uint32_t u = fill_unwritten ? UNWRITTEN : (0x3f000000u + (rnd() & 0xffffff)); memcpy(p + i, &u, 4); }
    if ((n * 4) % 16) __asan_poison_memory_region((char *)p + n * 4, 16 - (n * 4) % 16);
    return p;
}

// plane geometry of format F for a picture H x W: rows and bytes per row of each plane, pitches and offsets tight or padded
struct Planes { int n; int64_t rows[3], row_bytes[3]; };
template <class F>
static Planes planes_of(int H, int W)
{
    const int64_t cw = F::SUB == BSVD_SUB_444 ? W : W / 2, ch = F::SUB == BSVD_SUB_420 ? H / 2 : H;
    Planes p;
    p.n = F::PACKED ? 1 : F::LAY == BSVD_LAYOUT_SEMIPLANAR ? 2 : 3;
    p.rows[0] = H; p.rows[1] = p.rows[2] = ch;
    p.row_bytes[0] = F::PACKED ? 2 * W : (int64_t)W * F::SB;
    p.row_bytes[1] = (F::LAY == BSVD_LAYOUT_SEMIPLANAR ? 2 : 1) * cw * F::SB;
    p.row_bytes[2] = cw * F::SB;
    return p;
}
template <class F>
static SurfGeom geom_of(int H, int W, int Hp, int Wp, int cc, int pitched)
{
    const Planes p = planes_of<F>(H, W);
    SurfGeom g = {};
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.cc = cc; g.const_val = 0.125f;
    int64_t at = pitched ? 2 * 7 : 0;                            // plane 0 does not start the frame
    for (int i = 0; i < p.n; ++i) {
        g.pitch[i] = pitched ? (p.row_bytes[i] + 15) / 16 * 16 + 16 + 2 * i : p.row_bytes[i];
        g.off[i] = at;
        at += g.pitch[i] * p.rows[i] + (pitched ? 24 : 0);       // a gap behind every plane
    }
    g.fstride = at + (pitched ? 40 : 0);
    return g;
}

// NV12 / P010 as bsvd_yuv420_* describe them: one pitch for both planes, the CbCr plane directly behind the H rows of Y; pitched: rows padded
// to the next multiple of 64 bytes and 64 more, frames 128 bytes of slack apart
template <class F>
static SurfGeom geom_nv12(int H, int W, int Hp, int Wp, int cc, int pitched)
{
    const int64_t pitch = pitched ? ((int64_t)W * F::SB + 63) / 64 * 64 + 64 : (int64_t)W * F::SB;
    SurfGeom g = {};
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.cc = cc; g.const_val = 0.125f;
    g.pitch[0] = g.pitch[1] = pitch;
    g.off[1] = H * pitch;
    g.fstride = pitch * H * 3 / 2 + (pitched ? 128 : 0);
    return g;
}

// a surface of exactly its bytes: it ends at the last sample of the plane that ends last; with `poison` every byte that is no sample is poisoned
struct Surface { uint8_t *p; int64_t bytes; std::vector<uint8_t> is_sample; };
template <class F>
static Surface surface(int T, int H, int W, const SurfGeom &g, bool poison)
{
    const Planes pl = planes_of<F>(H, W);
    Surface s;
    int64_t end = 0;
    for (int i = 0; i < pl.n; ++i) { const int64_t e = g.off[i] + g.pitch[i] * (pl.rows[i] - 1) + pl.row_bytes[i]; if (e > end) end = e; }
    s.bytes = (int64_t)(T - 1) * g.fstride + end;
    s.p = (uint8_t *)malloc(s.bytes);
    s.is_sample.assign(s.bytes, 0);
    for (int64_t i = 0; i < s.bytes; ++i) s.p[i] = (uint8_t)rnd();
    if (poison) __asan_poison_memory_region(s.p, s.bytes);
    for (int f = 0; f < T; ++f)
        for (int i = 0; i < pl.n; ++i)
            for (int64_t r = 0; r < pl.rows[i]; ++r) {
                const int64_t at = f * g.fstride + g.off[i] + r * g.pitch[i];
                if (poison) __asan_unpoison_memory_region(s.p + at, pl.row_bytes[i]);
                memset(s.is_sample.data() + at, 1, pl.row_bytes[i]);
            }
    return s;
}
static void release(Surface &s) { __asan_unpoison_memory_region(s.p, s.bytes); free(s.p); }

using FNV12 = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_U8>;
using FP010 = SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>;

static const YuvDecode kDec8 = {16.f, 1.f / 219, 128.f, 1.f / 224, 1.5748f, 0.4681f, 0.1873f, 1.8556f};
static const YuvDecode kDec10 = {64.f, 1.f / 876, 512.f, 1.f / 896, 1.5748f, 0.4681f, 0.1873f, 1.8556f};
static const YuvEncode kEnc8 = {0.2126f, 0.7152f, 0.0722f, 219.f, 16.f, 120.7f, 142.2f, 128.f, 16.f, 235.f, 16.f, 240.f};
static const YuvEncode kEnc10 = {0.2126f, 0.7152f, 0.0722f, 876.f, 64.f, 482.9f, 568.9f, 512.f, 64.f, 940.f, 64.f, 960.f};

template <class F, int LINEAR>
static void surf_case(const char *name, int T, const SurfGeom &g)
{
    const int H = g.H, W = g.W, Hp = g.Hp, Wp = g.Wp;
    const int64_t plane = (int64_t)Hp * Wp, items = (int64_t)T * surf_item_rows<F>(H) * items_per_row(W);
    const YuvDecode kd = F::SB == 2 ? kDec10 : kDec8;
    const YuvEncode ke = F::SB == 2 ? kEnc10 : kEnc8;
    Surface s = surface<F>(T, H, W, g, true);
    float *dst = alloc_planes((int64_t)T * 4 * plane, true), *dst2 = alloc_planes((int64_t)T * 4 * plane, true);
    for (int64_t i = 0; i < items; ++i) yuv_to_planar_item<F, LINEAR>(s.p, dst, g, kd, i);
    for (int64_t f = 0; f < (int64_t)T * 4; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x) {
                const uint32_t got = bits_of(dst[f * plane + (int64_t)r * Wp + x]), from = bits_of(dst[f * plane + (int64_t)refl(r, H) * Wp + refl(x, W)]);
                EXPECT(got != UNWRITTEN, "%s in  lin%d %dx%d->%dx%d: (%d,%d,%d) not written", name, LINEAR, H, W, Hp, Wp, (int)f, r, x);
                EXPECT(got == from, "%s in  lin%d %dx%d->%dx%d: (%d,%d,%d) is not its mirror source", name, LINEAR, H, W, Hp, Wp, (int)f, r, x);
                if (f % 4 == 3) EXPECT(got == bits_of(0.125f), "%s in: constant channel", name);
            }
    if (F::SB == 2) {                                            // flip the 6 ignored bits of every word: the same tensor
        for (int64_t i = 0; i + 1 < s.bytes; i += 2)
            if (s.is_sample[i]) { uint16_t w; memcpy(&w, s.p + i, 2); w ^= F::SMP == SMP_HIGH10 ? 0x3f : 0xfc00; memcpy(s.p + i, &w, 2); }
        for (int64_t i = 0; i < items; ++i) yuv_to_planar_item<F, LINEAR>(s.p, dst2, g, kd, i);
        EXPECT(memcmp(dst, dst2, (size_t)T * 4 * plane * 4) == 0, "%s in  lin%d %dx%d: ignored bits reach the tensor", name, LINEAR, H, W);
    }
    release(s);
    // out: twice, the pad region of y random, then NaN: same bytes; bytes that are no sample stay (poisoned, and compared)
    SurfGeom gc = g;
    gc.cc = 0;
    float *y = alloc_planes((int64_t)T * 3 * plane, false);
    Surface o1 = surface<F>(T, H, W, gc, true), o2 = surface<F>(T, H, W, gc, true);
    __asan_unpoison_memory_region(o2.p, o2.bytes);
    std::vector<uint8_t> before(o2.p, o2.p + o2.bytes);
    for (int64_t i = 0; i < o2.bytes; ++i) if (o2.is_sample[i]) o2.p[i] = 0xEE;
    for (int64_t i = 0; i < o1.bytes; ++i) if (o1.is_sample[i]) o1.p[i] = 0xEE;
    for (int64_t i = 0; i < items; ++i) planar_to_yuv_item<F, LINEAR>(y, o1.p, gc, ke, i);
    for (int64_t f = 0; f < (int64_t)T * 3; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x)
                if (r >= H || x >= W) { const uint32_t u = 0x7fc00000u; memcpy(y + f * plane + (int64_t)r * Wp + x, &u, 4); }
    for (int64_t i = 0; i < items; ++i) planar_to_yuv_item<F, LINEAR>(y, o2.p, gc, ke, i);
    __asan_unpoison_memory_region(o1.p, o1.bytes);
    int64_t differ = 0, touched = 0, low = 0;
    for (int64_t i = 0; i < o2.bytes; ++i) {
        if (o2.is_sample[i]) differ += o1.p[i] != o2.p[i];
        else touched += o2.p[i] != before[i];
    }
    if (F::SB == 2)
        for (int64_t i = 0; i + 1 < o2.bytes; i += 2)
            if (o2.is_sample[i]) { uint16_t w; memcpy(&w, o2.p + i, 2); low += (w & (F::SMP == SMP_HIGH10 ? 0x3f : 0xfc00)) != 0; }
    EXPECT(differ == 0, "%s out lin%d %dx%d<-%dx%d: pad values of y reach %lld sample bytes", name, LINEAR, H, W, Hp, Wp, (long long)differ);
    EXPECT(touched == 0, "%s out lin%d %dx%d<-%dx%d: %lld bytes that are no sample were written", name, LINEAR, H, W, Hp, Wp, (long long)touched);
    EXPECT(low == 0, "%s out lin%d %dx%d: %lld words with ignored bits set", name, LINEAR, H, W, (long long)low);
    release(o1); release(o2); free(y); free(dst); free(dst2);
}

// yuv420p / yuv420p10le against nv12 / p010 (FS) on the same samples: the same floats in, the same codes out -- the planar loads and stores
// against the semi-planar ones
template <class F, class FS, int LINEAR>
static void against_semi_planar(const char *name, int T, int H, int W, int Hp, int Wp)
{
    using S = typename F::S;
    const SurfGeom g = geom_of<F>(H, W, Hp, Wp, 0, 0), gs = geom_nv12<FS>(H, W, Hp, Wp, 0, 0);
    const int64_t fstride = gs.fstride, plane = (int64_t)Hp * Wp;
    const int64_t items = (int64_t)T * (H / 2) * items_per_row(W), n = (int64_t)T * fstride / F::SB;
    const YuvDecode kd = F::SB == 2 ? kDec10 : kDec8;
    const YuvEncode ke = F::SB == 2 ? kEnc10 : kEnc8;
    std::vector<S> planar(n), semi(n);
    for (int f = 0; f < T; ++f) {
        S *p = planar.data() + f * (fstride / F::SB), *q = semi.data() + f * (fstride / F::SB);
        for (int64_t i = 0; i < (int64_t)H * W; ++i) { const unsigned c = rnd() & (F::SB == 2 ? 1023 : 255); p[i] = (S)c; q[i] = (S)(F::SB == 2 ? c << 6 : c); }
        for (int64_t r = 0; r < H / 2; ++r)
            for (int64_t x = 0; x < W / 2; ++x)
                for (int c = 0; c < 2; ++c) {
                    const unsigned v = rnd() & (F::SB == 2 ? 1023 : 255);
                    p[(int64_t)H * W + c * (H / 2) * (W / 2) + r * (W / 2) + x] = (S)v;
                    q[(int64_t)H * W + r * W + 2 * x + c] = (S)(F::SB == 2 ? v << 6 : v);
                }
    }
    float *a = alloc_planes((int64_t)T * 3 * plane, true), *b = alloc_planes((int64_t)T * 3 * plane, true);
    for (int64_t i = 0; i < items; ++i) {
        yuv_to_planar_item<F, LINEAR>((const uint8_t *)planar.data(), a, g, kd, i);
        yuv_to_planar_item<FS, LINEAR>((const uint8_t *)semi.data(), b, gs, kd, i);
    }
    EXPECT(memcmp(a, b, (size_t)T * 3 * plane * 4) == 0, "%s lin%d %dx%d->%dx%d: decode differs from the semi-planar format's", name, LINEAR, H, W, Hp, Wp);
    float *y = alloc_planes((int64_t)T * 3 * plane, false);
    for (int64_t i = 0; i < (int64_t)T * 3 * plane; ++i) y[i] = (float)((int)(rnd() % 1400) - 200) / 1000.f;      // out of gamut on both sides
    std::vector<S> op(n), os(n);
    for (int64_t i = 0; i < items; ++i) {
        planar_to_yuv_item<F, LINEAR>(y, (uint8_t *)op.data(), g, ke, i);
        planar_to_yuv_item<FS, LINEAR>(y, (uint8_t *)os.data(), gs, ke, i);
    }
    int64_t bad = 0;
    for (int f = 0; f < T; ++f) {
        const S *p = op.data() + f * (fstride / F::SB), *q = os.data() + f * (fstride / F::SB);
        for (int64_t i = 0; i < (int64_t)H * W; ++i) bad += (F::SB == 2 ? p[i] << 6 : p[i]) != q[i];
        for (int64_t r = 0; r < H / 2; ++r)
            for (int64_t x = 0; x < W / 2; ++x)
                for (int c = 0; c < 2; ++c) {
                    const unsigned v = p[(int64_t)H * W + c * (H / 2) * (W / 2) + r * (W / 2) + x];
                    bad += (F::SB == 2 ? v << 6 : v) != q[(int64_t)H * W + r * W + 2 * x + c];
                }
    }
    EXPECT(bad == 0, "%s lin%d %dx%d<-%dx%d: %lld codes differ from the semi-planar format's", name, LINEAR, H, W, Hp, Wp, (long long)bad);
    free(a); free(b); free(y);
}

template <class F, bool NV12 = false>
static void both(const char *name, const int (*sizes)[4], int n)
{
    for (int i = 0; i < n; ++i)
        for (int pitched = 0; pitched < 2; ++pitched) {
            const SurfGeom g = (NV12 ? geom_nv12<F> : geom_of<F>)(sizes[i][0], sizes[i][1], sizes[i][2], sizes[i][3], 1, pitched);
            surf_case<F, 0>(name, 2, g);
            if (F::SUB != BSVD_SUB_444) surf_case<F, 1>(name, 2, g);
        }
}

int main()
{
    // H, W, Hp, Wp: no pad, the issue's pad pictures, one item, half items, a pad of H - 1 rows and W - 1 columns
    const int s420[][4] = {{4, 4, 4, 4}, {8, 12, 8, 12}, {36, 52, 36, 52}, {6, 10, 8, 12}, {2, 6, 2, 8}, {6, 6, 8, 8}, {30, 42, 32, 44}, {6, 10, 10, 16}, {4, 6, 6, 8}};
    const int s422[][4] = {{4, 4, 4, 4}, {8, 12, 8, 12}, {36, 52, 36, 52}, {5, 10, 8, 12}, {2, 4, 3, 4}, {3, 6, 5, 8}, {7, 42, 8, 44}, {5, 10, 9, 16}, {9, 14, 9, 16}};
    const int s444[][4] = {{4, 4, 4, 4}, {8, 12, 8, 12}, {36, 52, 36, 52}, {5, 7, 8, 8}, {2, 3, 3, 4}, {3, 5, 5, 8}, {7, 41, 8, 44}, {5, 9, 9, 16}, {9, 13, 9, 16}, {3, 6, 4, 8}, {3, 3, 4, 4}};
    both<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_U8>>("yuv420p", s420, 9);
    both<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_LOW10>>("yuv420p10le", s420, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_UYVY, SMP_U8>>("uyvy422", s422, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_YUYV, SMP_U8>>("yuyv422", s422, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_SEMIPLANAR, SMP_U8>>("nv16", s422, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_SEMIPLANAR, SMP_HIGH10>>("p210le", s422, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_PLANAR, SMP_U8>>("yuv422p", s422, 9);
    both<SurfFmt<BSVD_SUB_422, BSVD_LAYOUT_PLANAR, SMP_LOW10>>("yuv422p10le", s422, 9);
    both<SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_U8>>("yuv444p", s444, 11);
    both<SurfFmt<BSVD_SUB_444, BSVD_LAYOUT_PLANAR, SMP_LOW10>>("yuv444p10le", s444, 11);
    // nv12 / p010 with the geometry of bsvd_yuv420_*: the sizes above and those the pad / crop bodies were first written against
    const int snv[][4] = {{8, 12, 12, 16}, {34, 52, 36, 52}, {10, 14, 16, 24}};
    both<FNV12, true>("nv12", s420, 9);
    both<FNV12, true>("nv12", snv, 3);
    both<FP010, true>("p010", s420, 9);
    both<FP010, true>("p010", snv, 3);
    for (const auto &s : s420) {
        against_semi_planar<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_U8>, FNV12, 0>("yuv420p", 2, s[0], s[1], s[2], s[3]);
        against_semi_planar<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_U8>, FNV12, 1>("yuv420p", 2, s[0], s[1], s[2], s[3]);
        against_semi_planar<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_LOW10>, FP010, 0>("yuv420p10le", 2, s[0], s[1], s[2], s[3]);
        against_semi_planar<SurfFmt<BSVD_SUB_420, BSVD_LAYOUT_PLANAR, SMP_LOW10>, FP010, 1>("yuv420p10le", 2, s[0], s[1], s[2], s[3]);
    }
    printf("yuv_surface_bounds: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
