// frame_pad_bounds.hip -- runs the item bodies of the pad / crop frame I/O kernels (bsvd_amd/csrc/frame_items.h) on the HOST, over heap
// buffers of exactly the bytes the ABI promises, under AddressSanitizer.  A GPU run cannot show a read that is not used -- the tail of a half
// item, pitch padding, the bytes behind the last row of the last frame --; here every byte of a frame buffer that is not a picture sample
// is either outside the allocation or poisoned, so such a read or write stops the program.  It also checks what needs no model: every
// destination element written, pad elements bit-equal to their mirror source, untouched bytes untouched.  Host code only: no kernel is
// launched and no device is needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/frame_pad_bounds.hip -o build/frame_pad_bounds && build/frame_pad_bounds
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 12345;
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

// ---- uint8 ----------------------------------------------------------------------------------------------------------------------------
static void u8_case(int T, int C, int cc, int H, int W, int Hp, int Wp, int hwc, int rev)
{
    const int64_t nsrc = (int64_t)T * C * H * W, plane = (int64_t)Hp * Wp, ndst = (int64_t)T * (C + cc) * plane;
    uint8_t *src = (uint8_t *)malloc(nsrc);
    for (int64_t i = 0; i < nsrc; ++i) src[i] = (uint8_t)rnd();
    float *dst = alloc_planes(ndst, true);
    const U8Geom g = {C, cc, H, W, Hp, Wp, hwc, rev, (Wp & 3) == 0, 0.125f};
    const int64_t items = (int64_t)T * H * items_per_row(W);
    for (int64_t i = 0; i < items; ++i) u8_to_planar_pad_item(src, dst, g, i);
    for (int f = 0; f < T; ++f)
        for (int c = 0; c < C + cc; ++c)
            for (int r = 0; r < Hp; ++r)
                for (int x = 0; x < Wp; ++x) {
                    const int sr = refl(r, H), sx = refl(x, W);
                    const float want = c >= C ? 0.125f : (float)src[hwc ? (((int64_t)f * H + sr) * W + sx) * C + c : (((int64_t)f * C + c) * H + sr) * W + sx] / 255.0f;
                    const float got = dst[((int64_t)f * (C + cc) + c) * plane + (int64_t)r * Wp + x];
                    EXPECT(bits_of(got) == bits_of(want), "u8 in  T%d C%d+%d %dx%d->%dx%d hwc%d: (%d,%d,%d,%d)", T, C, cc, H, W, Hp, Wp, hwc, f, c, r, x);
                }
    // out: the padded tensor's picture region back to codes, pad region NaN
    float *y = alloc_planes((int64_t)T * C * plane, false);
    for (int64_t f = 0; f < (int64_t)T * C; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x)
                if (r >= H || x >= W) { const uint32_t u = 0x7fc00000u; memcpy(y + f * plane + (int64_t)r * Wp + x, &u, 4); }
    uint8_t *out = (uint8_t *)malloc(nsrc);
    memset(out, 0xA5, nsrc);
    std::vector<uint8_t> want(nsrc);
    for (int f = 0; f < T; ++f)
        for (int c = 0; c < C; ++c)
            for (int r = 0; r < H; ++r)
                for (int x = 0; x < W; ++x) {
                    const int co = rev ? C - 1 - c : c;
                    want[hwc ? (((int64_t)f * H + r) * W + x) * C + co : (((int64_t)f * C + co) * H + r) * W + x] = u8_code(y[((int64_t)f * C + c) * plane + (int64_t)r * Wp + x]);
                }
    for (int64_t i = 0; i < items; ++i) planar_to_u8_crop_item(y, out, g, i);
    EXPECT(memcmp(out, want.data(), nsrc) == 0, "u8 out T%d C%d %dx%d<-%dx%d hwc%d rev%d", T, C, H, W, Hp, Wp, hwc, rev);
    free(src); free(dst); free(y); free(out);
}

// ---- YUV 4:2:0 ------------------------------------------------------------------------------------------------------------------------
// a surface of exactly its bytes: the last row of the last frame ends at its last sample; pitch padding and the gaps between frames are poisoned
struct Surface { uint8_t *p; int64_t bytes; };
static Surface surface(int T, int H, int W, int sb, int64_t pitch, int64_t fstride, bool poison)
{
    Surface s;
    s.bytes = (int64_t)(T - 1) * fstride + pitch * (H * 3 / 2 - 1) + (int64_t)W * sb;
    s.p = (uint8_t *)malloc(s.bytes);
    for (int64_t i = 0; i < s.bytes; ++i) s.p[i] = (uint8_t)rnd();
    if (poison)
        for (int f = 0; f < T; ++f) {
            for (int r = 0; r < H * 3 / 2; ++r) {
                uint8_t *e = s.p + f * fstride + r * pitch + (int64_t)W * sb, *n = s.p + f * fstride + (r + 1) * pitch;
                if (n > s.p + s.bytes) n = s.p + s.bytes;
                if (n > e) __asan_poison_memory_region(e, n - e);
            }
            uint8_t *e = s.p + f * fstride + pitch * (H * 3 / 2), *n = s.p + (f + 1) * fstride;
            if (f + 1 < T && n > e) __asan_poison_memory_region(e, n - e);
        }
    return s;
}
static void release(Surface s) { __asan_unpoison_memory_region(s.p, s.bytes); free(s.p); }

template <int PIX, int LINEAR>
static void yuv_case(int T, int H, int W, int Hp, int Wp, int pitched)
{
    constexpr int SB = (int)sizeof(typename Pix<PIX>::S);
    const int64_t pitch = pitched ? ((int64_t)W * SB + 63) / 64 * 64 + 64 : (int64_t)W * SB;
    const int64_t fstride = pitched ? pitch * H * 3 / 2 + 128 : pitch * H * 3 / 2;
    const int64_t plane = (int64_t)Hp * Wp, items = (int64_t)T * (H / 2) * items_per_row(W);
    const YuvPadGeom g = {H, W, Hp, Wp, 1, pitch, fstride, 0.125f};
    const YuvDecode kd = {64.f, 1.f / 876, 512.f, 1.f / 896, 1.5748f, 0.4681f, 0.1873f, 1.8556f};
    Surface s = surface(T, H, W, SB, pitch, fstride, true);
    float *dst = alloc_planes((int64_t)T * 4 * plane, true);
    for (int64_t i = 0; i < items; ++i) yuv420_to_planar_pad_item<PIX, LINEAR>(s.p, dst, g, kd, i);
    for (int64_t f = 0; f < (int64_t)T * 4; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x) {
                const uint32_t got = bits_of(dst[f * plane + (int64_t)r * Wp + x]), from = bits_of(dst[f * plane + (int64_t)refl(r, H) * Wp + refl(x, W)]);
                EXPECT(got != UNWRITTEN, "yuv in  pix%d lin%d %dx%d->%dx%d: (%d,%d,%d) not written", PIX, LINEAR, H, W, Hp, Wp, (int)f, r, x);
                EXPECT(got == from, "yuv in  pix%d lin%d %dx%d->%dx%d: (%d,%d,%d) is not its mirror source", PIX, LINEAR, H, W, Hp, Wp, (int)f, r, x);
                if (f % 4 == 3) EXPECT(got == bits_of(0.125f), "yuv in: constant channel");
            }
    release(s);
    // out: twice, the pad region of y random, then NaN: same bytes; bytes that are no sample stay (they are poisoned: a write there stops the run)
    const YuvEncode ke = {0.2126f, 0.7152f, 0.0722f, 876.f, 64.f, 482.9f, 568.9f, 512.f, 64.f, 940.f, 64.f, 960.f};
    const YuvPadGeom gc = {H, W, Hp, Wp, 0, pitch, fstride, 0.f};
    float *y = alloc_planes((int64_t)T * 3 * plane, false);
    Surface o1 = surface(T, H, W, SB, pitch, fstride, true), o2 = surface(T, H, W, SB, pitch, fstride, true);
    for (int64_t i = 0; i < items; ++i) planar_to_yuv420_crop_item<PIX, LINEAR>(y, o1.p, gc, ke, i);
    for (int64_t f = 0; f < (int64_t)T * 3; ++f)
        for (int r = 0; r < Hp; ++r)
            for (int x = 0; x < Wp; ++x)
                if (r >= H || x >= W) { const uint32_t u = 0x7fc00000u; memcpy(y + f * plane + (int64_t)r * Wp + x, &u, 4); }
    for (int64_t i = 0; i < items; ++i) planar_to_yuv420_crop_item<PIX, LINEAR>(y, o2.p, gc, ke, i);
    for (int f = 0; f < T; ++f)
        for (int r = 0; r < H * 3 / 2; ++r)
            EXPECT(memcmp(o1.p + f * fstride + r * pitch, o2.p + f * fstride + r * pitch, (size_t)W * SB) == 0,
                   "yuv out pix%d lin%d %dx%d<-%dx%d: pad values of y reach row %d", PIX, LINEAR, H, W, Hp, Wp, r);
    release(o1); release(o2); free(y); free(dst);
}

int main()
{
    const int u8_sizes[][4] = {{3, 3, 4, 4}, {5, 7, 8, 8}, {30, 50, 32, 52}, {8, 12, 12, 16}, {8, 12, 8, 12}, {1, 1, 1, 1}, {2, 2, 3, 3}, {5, 6, 9, 11}, {6, 9, 6, 13}};
    for (const auto &s : u8_sizes)
        for (int hwc = 0; hwc < 2; ++hwc)
            for (int C : {1, 3, 4})
                for (int cc = 0; cc < 2; ++cc) u8_case(2, C, cc, s[0], s[1], s[2], s[3], hwc, cc);
    const int yuv_sizes[][4] = {{8, 12, 12, 16}, {36, 52, 36, 52}, {6, 6, 8, 8}, {6, 10, 8, 12}, {30, 42, 32, 44}, {34, 52, 36, 52}, {2, 6, 2, 8}, {4, 6, 6, 8}, {6, 10, 10, 16}};
    for (const auto &s : yuv_sizes)
        for (int pitched = 0; pitched < 2; ++pitched) {
            yuv_case<BSVD_PIX_NV12, 0>(2, s[0], s[1], s[2], s[3], pitched);
            yuv_case<BSVD_PIX_NV12, 1>(2, s[0], s[1], s[2], s[3], pitched);
            yuv_case<BSVD_PIX_P010, 0>(2, s[0], s[1], s[2], s[3], pitched);
            yuv_case<BSVD_PIX_P010, 1>(2, s[0], s[1], s[2], s[3], pitched);
        }
    printf("frame_pad_bounds: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
