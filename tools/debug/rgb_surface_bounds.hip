// rgb_surface_bounds.hip -- runs the item bodies of the RGB surface kernels (bsvd_amd/csrc/frame_rgb_items.h), all nine instantiations, on the
// HOST, over heap buffers of exactly the bytes the ABI promises, under AddressSanitizer, in the manner of yuv_surface_bounds.hip: every
// byte of a surface that is not a sample -- pitch padding, the bytes between planes and frames, the bytes behind the last sample -- is
// outside the allocation or poisoned, and so are the bytes around the fp32 tensors and the alpha planes, so a read or write there stops
// the program.  It also checks what needs no model: every destination element written, pad elements bit-equal to their mirror source,
// non-sample bytes untouched, NaN in the pad region of the fp32 tensor reaching no sample, the ignored bits of a word reaching no value,
// alpha out equal to alpha in, the vector and the scalar fp32 side giving the same bits.  Host code only: no kernel is launched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/rgb_surface_bounds.hip -o build/rgb_surface_bounds && build/rgb_surface_bounds
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_rgb_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 4321;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static const uint32_t UNWRITTEN = 0x7fc12345u;      // a NaN pattern no conversion produces
static int refl(int i, int N) { return i < N ? i : 2 * (N - 1) - i; }

// n floats of exactly their bytes, `lead` floats behind a 16-byte boundary (lead = 1: the tensor is not 16-byte aligned)
struct Planes { char *base; float *p; };
static Planes alloc_planes(int64_t n, bool fill_unwritten, int lead)
{
    const size_t bytes = (size_t)(((n + lead) * 4 + 15) / 16 * 16);
    Planes a;
    a.base = (char *)aligned_alloc(16, bytes);
    a.p = (float *)a.base + lead;
    for (int64_t i = 0; i < n; ++i) { const uint32_t u = fill_unwritten ? UNWRITTEN : (0x3f000000u + (rnd() & 0xffffff)); memcpy(a.p + i, &u, 4); }
    if (lead) __asan_poison_memory_region(a.base, lead * 4);
    if (bytes > (size_t)(n + lead) * 4) __asan_poison_memory_region((char *)(a.p + n), bytes - (size_t)(n + lead) * 4);
    return a;
}
static void release(Planes &a) { free(a.base); }

template <class F> static int plane_count() { return F::LAY == BSVD_RGB_PLANAR ? F::SLOTS : 1; }
template <class F> static int64_t row_bytes(int W) { return F::LAY == BSVD_RGB_PLANAR ? (int64_t)W * F::SB : F::LAY == BSVD_RGB_PACKED ? (int64_t)W * F::SB * F::SLOTS : (int64_t)W * 4; }

template <class F>
static RgbGeom geom_of(int H, int W, int Hp, int Wp, int cc, int pitched, int vec, int bits, int rot)
{
    RgbGeom g = {};
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.cc = cc; g.const_val = 0.125f; g.vec = vec;
    for (int j = 0; j < 4; ++j) g.chan[j] = j < F::SLOTS ? (j + rot) % F::SLOTS : 3;      // a rotated component order
    g.mask = (1u << bits) - 1;
    int64_t at = pitched ? 4 * 7 : 0;
    for (int i = 0; i < plane_count<F>(); ++i) {
        g.pitch[i] = pitched ? (row_bytes<F>(W) + 15) / 16 * 16 + 16 + 4 * i : row_bytes<F>(W);
        g.off[i] = at;
        at += g.pitch[i] * H + (pitched ? 24 : 0);
    }
    g.fstride = at + (pitched ? 40 : 0);
    return g;
}

// a surface of exactly its bytes: it ends at the last sample of the plane that ends last; every byte that is no sample is poisoned
struct Surface { uint8_t *p; int64_t bytes; std::vector<uint8_t> is_sample; };
template <class F>
static Surface surface(int T, const RgbGeom &g)
{
    Surface s;
    int64_t end = 0;
    for (int i = 0; i < plane_count<F>(); ++i) { const int64_t e = g.off[i] + g.pitch[i] * (g.H - 1) + row_bytes<F>(g.W); if (e > end) end = e; }
    s.bytes = (int64_t)(T - 1) * g.fstride + end;
    s.p = (uint8_t *)malloc(s.bytes);
    s.is_sample.assign(s.bytes, 0);
    for (int64_t i = 0; i < s.bytes; ++i) s.p[i] = (uint8_t)rnd();
    __asan_poison_memory_region(s.p, s.bytes);
    for (int f = 0; f < T; ++f)
        for (int i = 0; i < plane_count<F>(); ++i)
            for (int64_t r = 0; r < g.H; ++r) {
                const int64_t at = f * g.fstride + g.off[i] + r * g.pitch[i];
                __asan_unpoison_memory_region(s.p + at, row_bytes<F>(g.W));
                memset(s.is_sample.data() + at, 1, row_bytes<F>(g.W));
            }
    return s;
}
static void release(Surface &s) { __asan_unpoison_memory_region(s.p, s.bytes); free(s.p); }

template <class F>
static void rgb_case(const char *name, int T, int bits, const int size[4], int pitched, int rot)
{
    using A = typename F::A;
    const int H = size[0], W = size[1], Hp = size[2], Wp = size[3];
    const int64_t plane = (int64_t)Hp * Wp, items = (int64_t)T * H * items_per_row(W), pic = (int64_t)T * H * W;
    const bool four = F::SLOTS == 4;
    const float s = (float)(1 << (bits - 8));
    const RgbDecode kd = {16.f * s, 219.f * s};
    const RgbEncode ke = {219.f * s, 16.f * s, 16.f * s, 235.f * s, (1u << bits) - 1};
    Planes first = {};
    std::vector<A> alpha_first;
    for (int vec = (Wp & 3) == 0; vec >= 0; --vec) {                  // the float4 side (tensor aligned), then the scalar side (4 bytes off)
        const RgbGeom g = geom_of<F>(H, W, Hp, Wp, 1, pitched, vec, bits, rot);
        Surface sf = surface<F>(T, g);
        A *alpha = (A *)malloc(pic * sizeof(A));
        memset(alpha, 0xEE, pic * sizeof(A));
        Planes dst = alloc_planes((int64_t)T * 4 * plane, true, vec ? 0 : 1), dst2 = alloc_planes((int64_t)T * 4 * plane, true, vec ? 0 : 1);
        rng_state = 99 + bits;                                        // the same samples for both sides
        for (int64_t i = 0; i < sf.bytes; ++i) if (sf.is_sample[i]) sf.p[i] = (uint8_t)rnd();
        for (int64_t i = 0; i < items; ++i) rgb_to_planar_item<F>(sf.p, dst.p, four ? alpha : nullptr, g, kd, i);
        for (int64_t f = 0; f < (int64_t)T * 4; ++f)
            for (int r = 0; r < Hp; ++r)
                for (int x = 0; x < Wp; ++x) {
                    const uint32_t got = bits_of(dst.p[f * plane + (int64_t)r * Wp + x]), from = bits_of(dst.p[f * plane + (int64_t)refl(r, H) * Wp + refl(x, W)]);
                    EXPECT(got != UNWRITTEN, "%s in  vec%d %dx%d->%dx%d: (%d,%d,%d) not written", name, vec, H, W, Hp, Wp, (int)f, r, x);
                    EXPECT(got == from, "%s in  vec%d %dx%d->%dx%d: (%d,%d,%d) is not its mirror source", name, vec, H, W, Hp, Wp, (int)f, r, x);
                    if (f % 4 == 3) EXPECT(got == bits_of(0.125f), "%s in: constant channel", name);
                }
        if (first.p) EXPECT(memcmp(first.p, dst.p, (size_t)T * 4 * plane * 4) == 0, "%s in  %dx%d->%dx%d: the scalar side differs from the float4 side", name, H, W, Hp, Wp);
        if (four) {
            for (int64_t i = 0; i < pic; ++i) EXPECT((unsigned)alpha[i] <= g.mask, "%s in: alpha code %lld above the mask (or not written)", name, (long long)i);
            if (!alpha_first.empty()) EXPECT(memcmp(alpha_first.data(), alpha, pic * sizeof(A)) == 0, "%s in: alpha differs between the sides", name);
            alpha_first.assign(alpha, alpha + pic);
        }
        // flip every ignored bit: the same tensor
        const unsigned ignored = F::LAY == BSVD_RGB_PACKED_X2_10 ? 0xc0000000u : F::SB == 2 ? (~g.mask & 0xffffu) : 0u;
        if (ignored) {
            for (int64_t i = 0; i + (int64_t)sizeof(typename F::S) <= sf.bytes; i += sizeof(typename F::S))
                if (sf.is_sample[i]) { typename F::S w; memcpy(&w, sf.p + i, sizeof(w)); w ^= (typename F::S)ignored; memcpy(sf.p + i, &w, sizeof(w)); }
            for (int64_t i = 0; i < items; ++i) rgb_to_planar_item<F>(sf.p, dst2.p, nullptr, g, kd, i);
            EXPECT(memcmp(dst.p, dst2.p, (size_t)T * 4 * plane * 4) == 0, "%s in  %dx%d: ignored bits reach the tensor", name, H, W);
        }
        release(sf);
        // out: twice, the pad region of y random, then NaN: same bytes; bytes that are no sample stay (poisoned, and compared)
        RgbGeom gc = g;
        gc.cc = 0;
        Planes y = alloc_planes((int64_t)T * 3 * plane, false, vec ? 0 : 1);
        Surface o1 = surface<F>(T, gc), o2 = surface<F>(T, gc);
        __asan_unpoison_memory_region(o2.p, o2.bytes);
        std::vector<uint8_t> before(o2.p, o2.p + o2.bytes);
        for (int64_t i = 0; i < o2.bytes; ++i) if (!o2.is_sample[i]) __asan_poison_memory_region(o2.p + i, 1);
        for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(y.p, o1.p, four ? alpha : nullptr, gc, ke, i);
        for (int64_t f = 0; f < (int64_t)T * 3; ++f)
            for (int r = 0; r < Hp; ++r)
                for (int x = 0; x < Wp; ++x)
                    if (r >= H || x >= W) { const uint32_t u = 0x7fc00000u; memcpy(y.p + f * plane + (int64_t)r * Wp + x, &u, 4); }
        for (int64_t i = 0; i < items; ++i) planar_to_rgb_item<F>(y.p, o2.p, four ? alpha : nullptr, gc, ke, i);
        __asan_unpoison_memory_region(o1.p, o1.bytes);
        __asan_unpoison_memory_region(o2.p, o2.bytes);
        int64_t differ = 0, touched = 0, high = 0;
        for (int64_t i = 0; i < o2.bytes; ++i) {
            if (o2.is_sample[i]) differ += o1.p[i] != o2.p[i];
            else touched += o2.p[i] != before[i];
        }
        if (F::LAY != BSVD_RGB_PACKED_X2_10 && F::SB == 2)
            for (int64_t i = 0; i + 1 < o2.bytes; i += 2)
                if (o2.is_sample[i]) { uint16_t w; memcpy(&w, o2.p + i, 2); high += (w & ~g.mask) != 0; }
        EXPECT(differ == 0, "%s out vec%d %dx%d<-%dx%d: pad values of y reach %lld sample bytes", name, vec, H, W, Hp, Wp, (long long)differ);
        EXPECT(touched == 0, "%s out vec%d %dx%d<-%dx%d: %lld bytes that are no sample were written", name, vec, H, W, Hp, Wp, (long long)touched);
        EXPECT(high == 0, "%s out %dx%d: %lld words with ignored bits set", name, H, W, (long long)high);
        if (four) {                                                   // alpha out = alpha in
            Planes back = alloc_planes((int64_t)T * 3 * plane, true, vec ? 0 : 1);
            std::vector<A> a2(pic);
            gc.cc = 0;
            for (int64_t i = 0; i < items; ++i) rgb_to_planar_item<F>(o2.p, back.p, a2.data(), gc, kd, i);
            EXPECT(memcmp(a2.data(), alpha, pic * sizeof(A)) == 0, "%s: alpha does not come back", name);
            release(back);
        }
        release(o1); release(o2); release(y); release(dst2); free(alpha);
        if (first.p) { release(first); first.p = nullptr; release(dst); } else first = dst;
    }
    if (first.p) release(first);
}

template <class F>
static void all_sizes(const char *name, int bits)
{
    // H, W, Hp, Wp: whole items, the tests' pad pictures, the scalar fp32 side with the largest pad, one pixel, part items of 1, 2, 3
    const int sizes[][4] = {{4, 4, 4, 4}, {4, 12, 4, 12}, {36, 52, 36, 52}, {5, 7, 8, 8}, {6, 10, 8, 12}, {5, 7, 9, 9}, {1, 1, 1, 1}, {2, 5, 3, 8}, {3, 6, 5, 11},
                            {7, 41, 8, 44}, {3, 3, 4, 4}};
    for (const auto &s : sizes)
        for (int pitched = 0; pitched < 2; ++pitched)
            rgb_case<F>(name, 2, bits, s, pitched, (s[0] + pitched) % F::SLOTS);
}

int main()
{
    all_sizes<RgbFmt<BSVD_RGB_PACKED, 1, 3>>("packed 8 x 3", 8);
    all_sizes<RgbFmt<BSVD_RGB_PACKED, 1, 4>>("packed 8 x 4", 8);
    all_sizes<RgbFmt<BSVD_RGB_PACKED, 2, 3>>("packed 16 x 3", 16);
    all_sizes<RgbFmt<BSVD_RGB_PACKED, 2, 4>>("packed 16 x 4", 16);
    all_sizes<RgbFmt<BSVD_RGB_PACKED, 2, 4>>("packed 12 x 4", 12);
    all_sizes<RgbFmt<BSVD_RGB_PACKED_X2_10, 4, 3>>("x2 10", 10);
    all_sizes<RgbFmt<BSVD_RGB_PLANAR, 1, 3>>("planar 8 x 3", 8);
    all_sizes<RgbFmt<BSVD_RGB_PLANAR, 1, 4>>("planar 8 x 4", 8);
    all_sizes<RgbFmt<BSVD_RGB_PLANAR, 2, 3>>("planar 10 x 3", 10);
    all_sizes<RgbFmt<BSVD_RGB_PLANAR, 2, 4>>("planar 12 x 4", 12);
    all_sizes<RgbFmt<BSVD_RGB_PLANAR, 2, 4>>("planar 16 x 4", 16);
    printf("rgb_surface_bounds: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
