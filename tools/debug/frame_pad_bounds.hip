// frame_pad_bounds.hip -- runs the item bodies of the uint8 pad / crop frame I/O kernels (bsvd_amd/csrc/frame_items.h) on the HOST, over heap
// buffers of exactly the bytes the ABI promises, under AddressSanitizer.  A GPU run cannot show a read that is not used -- the tail of a part
// item, the bytes behind the last row of the last frame --; here such a read or write lies outside the allocation and stops the program.
// It also checks what needs no model: every destination element written, pad elements bit-equal to their mirror source, untouched bytes
// untouched.  The YUV bodies, NV12 and P010 among them, have yuv_surface_bounds.hip.  Host code only: no kernel is launched and no device
// is needed.
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

int main()
{
    const int u8_sizes[][4] = {{3, 3, 4, 4}, {5, 7, 8, 8}, {30, 50, 32, 52}, {8, 12, 12, 16}, {8, 12, 8, 12}, {1, 1, 1, 1}, {2, 2, 3, 3}, {5, 6, 9, 11}, {6, 9, 6, 13}};
    for (const auto &s : u8_sizes)
        for (int hwc = 0; hwc < 2; ++hwc)
            for (int C : {1, 3, 4})
                for (int cc = 0; cc < 2; ++cc) u8_case(2, C, cc, s[0], s[1], s[2], s[3], hwc, cc);
    printf("frame_pad_bounds: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
