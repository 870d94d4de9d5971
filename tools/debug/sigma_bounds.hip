// sigma_bounds.hip -- runs the item bodies of the noise-level estimate (bsvd_amd/csrc/frame_sigma_items.h) on the HOST, over heap buffers of
// exactly the floats the ABI promises, under AddressSanitizer, in the manner of frame_pad_bounds.hip / yuv_surface_bounds.hip: a read
// before the first row, behind the last row of the last plane the estimate pools, or a fill store outside its plane stops the program.  It
// also checks what needs no model: the items' histogram equals a plain loop over the interior pixels, NaN outside the picture reaches no
// count, the serial finish on a one-bin histogram, and the fill writes its plane and nothing else.  Host code only: no kernel is launched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/sigma_bounds.hip -o build/sigma_bounds && build/sigma_bounds
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_sigma_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 99;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct HostAdd {
    uint32_t *h;
    void operator()(int q, bool counted) { if (counted) ++h[q]; }
};

// frames x channels planes of Hp x Wp, and not one float more: the estimate may read no plane behind them
static void run(int frames, int ch, int H, int W, int Hp, int Wp, int nan_outside)
{
    const int64_t plane = (int64_t)Hp * Wp, n = (int64_t)frames * ch * plane;
    float *x = (float *)aligned_alloc(16, (size_t)((n * 4 + 15) / 16 * 16));
    for (int64_t i = 0; i < n; ++i) x[i] = (float)(rnd() & 255) * (1.f / 255.f);
    if (nan_outside)
        for (int64_t i = 0; i < n; ++i) { const int r = (int)(i % plane) / Wp, c = (int)(i % plane) % Wp; if (r >= H || c >= W) x[i] = NAN; }
    SigmaGeom g;
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.ch = ch; g.fstride = ch * plane;
    for (int vec = 0; vec <= ((Wp & 3) || (g.fstride & 3) ? 0 : 1); ++vec) {
        g.vec = vec;
        for (int f = 0; f < frames; ++f) {
            std::vector<uint32_t> got(SIGMA_BINS, 0), want(SIGMA_BINS, 0);
            HostAdd add{got.data()};
            const float *fr = x + f * g.fstride;
            for (int i = 0; i < (int)sigma_items(g); ++i) sigma_hist_item(fr, g, i, add);
            int64_t counted = 0;
            for (int c = 0; c < ch; ++c)
                for (int r = 1; r <= H - 2; ++r)
                    for (int col = 1; col <= W - 2; ++col) {
                        const float *p = fr + c * plane + (int64_t)r * Wp + col;
                        const float resp = (4.f * p[0] - 2.f * ((p[-Wp] + p[Wp]) + (p[-1] + p[1]))) + ((p[-Wp - 1] + p[-Wp + 1]) + (p[Wp - 1] + p[Wp + 1]));
                        int q;
                        if (sigma_bin(resp, &q)) { ++want[q]; ++counted; }
                    }
            EXPECT(got == want, "%d x %d x %d x %d in %d x %d vec %d frame %d: histogram differs from the plain loop", frames, ch, H, W, Hp, Wp, vec, f);
            EXPECT(counted == (int64_t)ch * (H - 2) * (W - 2), "%d x %d in %d x %d: %lld samples counted", H, W, Hp, Wp, (long long)counted);
            const float s = sigma_finish_serial(got.data(), 1.f, 0.f, 1.f);
            EXPECT(s >= 0.f && s <= 1.f, "sigma %g outside the clamp", s);
        }
    }
    free(x);
}

static void run_fill(int frames, int C, int Hp, int Wp)
{
    const int64_t n = (int64_t)Hp * Wp, all = (int64_t)frames * C * n;
    float *x = (float *)aligned_alloc(16, (size_t)((all * 4 + 15) / 16 * 16));
    for (int64_t i = 0; i < all; ++i) x[i] = -1.f;
    const int vec = !(n & 3);
    for (int f = 0; f < frames; ++f)
        for (int64_t i = 0; i < (n + 3) / 4; ++i) sigma_fill_item(x + (f * C + C - 1) * n, n, i, 0.25f + f, vec);
    for (int64_t i = 0; i < all; ++i) {
        const int f = (int)(i / (C * n)), c = (int)(i / n) % C;
        EXPECT(x[i] == (c == C - 1 ? 0.25f + f : -1.f), "fill %d x %d x %d x %d: element %lld = %g", frames, C, Hp, Wp, (long long)i, x[i]);
    }
    free(x);
}

int main()
{
    const int sizes[][4] = {{3, 3, 3, 3}, {4, 4, 4, 4}, {12, 20, 12, 20}, {37, 53, 40, 56}, {5, 6, 7, 9}, {9, 67, 9, 67}, {10, 8, 10, 8},
                            {11, 5, 11, 5}, {19, 3, 19, 3}, {17, 21, 17, 24}, {8, 9, 8, 12}, {7, 13, 9, 13}};
    for (auto &s : sizes)
        for (int nan_outside = 0; nan_outside <= 1; ++nan_outside) run(2, 3, s[0], s[1], s[2], s[3], nan_outside);
    run(1, 1, 3, 3, 3, 3, 0);
    run_fill(2, 4, 5, 7);
    run_fill(2, 4, 12, 20);
    run_fill(3, 2, 1, 1);
    uint32_t h[SIGMA_BINS] = {};
    EXPECT(sigma_finish_serial(h, 1.f, 0.125f, 1.f) == 0.125f, "empty histogram does not give lo");
    h[100] = 7;
    EXPECT(sigma_finish_serial(h, 1.f, 0.f, 1.f) == (float)(100.5 * SIGMA_K), "one-bin histogram: median not in the middle of the bin");
    printf(failures ? "sigma_bounds: %d FAILURES\n" : "sigma_bounds: ok\n", failures);
    return failures != 0;
}
