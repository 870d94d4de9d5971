// nlf_bounds.hip -- runs the item bodies of the noise-level function (bsvd_amd/csrc/frame_nlf_items.h) on the HOST, over heap buffers of
// exactly the floats the ABI promises, under AddressSanitizer, in the manner of sigma_bounds.hip: a read before the first row, behind the
// last row of the third plane, or a map store outside its plane stops the program.  It also checks what needs no model: the items'
// histogram equals a plain loop over the interior pixels, NaN outside the picture reaches no count, the level-summed histogram equals
// sigma_hist_item's bins summed in fours, the serial finish on hand-built histograms, a flat curve gives its value at every pixel, the map
// is finite over NaN / Inf planes and writes its plane and nothing else.  Host code only: no kernel is launched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address -Iinclude -Ibsvd_amd/csrc \
//         tools/debug/nlf_bounds.hip -o build/nlf_bounds && build/nlf_bounds
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_nlf_items.h"

using namespace bsvd;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 77;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct HostAdd {
    uint32_t *h;
    void operator()(int q, bool counted) { if (counted) ++h[q]; }
};

// frames x 3 planes of Hp x Wp, and not one float more: the estimate may read no plane behind them
static void run_hist(int frames, int H, int W, int Hp, int Wp, int nan_outside)
{
    const int64_t plane = (int64_t)Hp * Wp, n = (int64_t)frames * 3 * plane;
    float *x = (float *)aligned_alloc(16, (size_t)((n * 4 + 15) / 16 * 16));
    for (int64_t i = 0; i < n; ++i) x[i] = (float)(rnd() & 255) * (1.f / 255.f);
    if (nan_outside)
        for (int64_t i = 0; i < n; ++i) { const int r = (int)(i % plane) / Wp, c = (int)(i % plane) % Wp; if (r >= H || c >= W) x[i] = NAN; }
    SigmaGeom g;
    g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.ch = 3; g.fstride = 3 * plane;
    for (int vec = 0; vec <= ((Wp & 3) || (g.fstride & 3) ? 0 : 1); ++vec) {
        g.vec = vec;
        for (int f = 0; f < frames; ++f) {
            std::vector<uint32_t> got(NLF_HIST, 0), want(NLF_HIST, 0), fine(SIGMA_BINS, 0);
            HostAdd add{got.data()}, add_fine{fine.data()};
            const float *fr = x + f * g.fstride;
            for (int i = 0; i < (int)sigma_items(g); ++i) { nlf_hist_item(fr, g, i, add); sigma_hist_item(fr, g, i, add_fine); }
            int64_t counted = 0;
            for (int c = 0; c < 3; ++c)
                for (int r = 1; r <= H - 2; ++r)
                    for (int col = 1; col <= W - 2; ++col) {
                        const float *p = fr + c * plane + (int64_t)r * Wp + col;
                        const float resp = (4.f * p[0] - 2.f * ((p[-Wp] + p[Wp]) + (p[-1] + p[1]))) + ((p[-Wp - 1] + p[-Wp + 1]) + (p[Wp - 1] + p[Wp + 1]));
                        const float S = ((((p[-Wp - 1] + p[-Wp]) + p[-Wp + 1]) + ((p[-1] + p[0]) + p[1])) + ((p[Wp - 1] + p[Wp]) + p[Wp + 1]));
                        int q;
                        if (nlf_bin(resp, &q)) { ++want[nlf_level(S) * NLF_BINS + q]; ++counted; }
                    }
            EXPECT(got == want, "%d x %d x %d in %d x %d vec %d frame %d: histogram differs from the plain loop", frames, H, W, Hp, Wp, vec, f);
            EXPECT(counted == (int64_t)3 * (H - 2) * (W - 2), "%d x %d in %d x %d: %lld samples counted", H, W, Hp, Wp, (long long)counted);
            for (int k = 0; k < NLF_BINS; ++k) {
                uint32_t a = 0, b = 0;
                for (int l = 0; l < NLF_LEVELS; ++l) a += got[l * NLF_BINS + k];
                for (int j = 0; j < 4; ++j) b += fine[4 * k + j];
                if (a != b) { EXPECT(false, "%d x %d: level-summed bin %d = %u, the scalar estimate's four bins = %u", H, W, k, a, b); break; }
            }
            float curve[NLF_LEVELS];
            nlf_finish_serial(got.data(), 1.f, 0.f, 1.f, 8, curve);
            for (int l = 0; l < NLF_LEVELS; ++l) EXPECT(curve[l] >= 0.f && curve[l] <= 1.f, "curve[%d] = %g outside the clamp", l, curve[l]);
        }
    }
    free(x);
}

// frames x C planes of Hp x Wp exactly; kind 0: codes, 1: NaN / Inf / huge values among them
static void run_map(int frames, int C, int Hp, int Wp, int kind)
{
    const int64_t n = (int64_t)Hp * Wp, all = (int64_t)frames * C * n;
    float *x = (float *)aligned_alloc(16, (size_t)((all * 4 + 15) / 16 * 16));
    std::vector<float> before((size_t)all);
    for (int64_t i = 0; i < all; ++i) {
        x[i] = (float)(rnd() & 255) * (1.f / 255.f);
        if (kind == 1 && rnd() % 7 == 0) { const float bad[5] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f}; x[i] = bad[rnd() % 5]; }
    }
    for (int f = 0; f < frames; ++f)
        for (int64_t i = 0; i < n; ++i) x[(f * C + C - 1) * n + i] = NAN;
    memcpy(before.data(), x, (size_t)all * 4);
    float ramp[NLF_LEVELS], flat[NLF_LEVELS];
    for (int l = 0; l < NLF_LEVELS; ++l) { ramp[l] = 0.01f + 0.003f * l * l; flat[l] = 0.0625f; }
    NlfMapGeom g;
    g.Hp = Hp; g.Wp = Wp; g.out_plane = C - 1; g.fstride = C * n;
    for (int pass = 0; pass < 2; ++pass)
        for (int vec = 0; vec <= ((Wp & 3) || (g.fstride & 3) ? 0 : 1); ++vec) {
            g.vec = vec;
            const float *curve = pass ? flat : ramp;
            for (int f = 0; f < frames; ++f)
                for (int64_t i = 0; i < nlf_map_items(g); ++i) nlf_map_item(x + f * g.fstride, g, curve, i);
            for (int64_t i = 0; i < all; ++i) {
                const int c = (int)(i / n) % C;
                if (c != C - 1) { EXPECT(memcmp(&x[i], &before[(size_t)i], 4) == 0, "map %d x %d x %d x %d: colour element %lld changed", frames, C, Hp, Wp, (long long)i); continue; }
                EXPECT(x[i] >= ramp[0] && x[i] <= ramp[NLF_LEVELS - 1] * 1.0001f, "map %d x %d x %d x %d kind %d: element %lld = %g", frames, C, Hp, Wp, kind, (long long)i, x[i]);
                if (pass) EXPECT(x[i] == 0.0625f, "flat curve: element %lld = %g", (long long)i, x[i]);
            }
            for (int f = 0; f < frames; ++f)
                for (int64_t i = 0; i < n; ++i) x[(f * C + C - 1) * n + i] = NAN;
        }
    free(x);
}

int main()
{
    const int sizes[][4] = {{3, 3, 3, 3}, {4, 4, 4, 4}, {12, 20, 12, 20}, {37, 50, 40, 52}, {5, 6, 7, 9}, {9, 67, 9, 67}, {10, 8, 10, 8},
                            {11, 5, 11, 5}, {19, 3, 19, 3}, {17, 21, 17, 24}, {8, 9, 8, 12}, {7, 13, 9, 13}};
    for (auto &s : sizes)
        for (int nan_outside = 0; nan_outside <= 1; ++nan_outside) run_hist(2, s[0], s[1], s[2], s[3], nan_outside);
    const int planes[][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 3}, {5, 7}, {12, 20}, {40, 52}, {9, 13}, {8, 12}, {17, 4}, {16, 8}};
    for (auto &p : planes)
        for (int kind = 0; kind <= 1; ++kind) { run_map(2, 4, p[0], p[1], kind); run_map(1, 5, p[0], p[1], kind); }

    std::vector<uint32_t> h(NLF_HIST, 0);
    float c[NLF_LEVELS];
    nlf_finish_serial(h.data(), 1.f, 0.125f, 1.f, 512, c);
    for (int l = 0; l < NLF_LEVELS; ++l) EXPECT(c[l] == 0.125f, "empty histogram: level %d = %g, not lo", l, c[l]);
    h[2 * NLF_BINS + 20] = 600; h[6 * NLF_BINS + 80] = 600;                 // levels 2 and 6 valid: 4 ties to the lower one
    nlf_finish_serial(h.data(), 1.f, 0.f, 1.f, 512, c);
    const float lo2 = (float)(20.5 * NLF_K), hi6 = (float)(80.5 * NLF_K);
    for (int l = 0; l < NLF_LEVELS; ++l) EXPECT(c[l] == (l <= 4 ? lo2 : hi6), "nearest-valid fill: level %d = %g", l, c[l]);
    nlf_finish_serial(h.data(), 1.f, 0.f, 1.f, 600, c);
    EXPECT(c[2] == lo2 && c[6] == hi6, "min_count = N is valid");
    nlf_finish_serial(h.data(), 1.f, 0.f, 1.f, 601, c);                      // no level valid: pooled, 2 cum = N at the end of bin 20
    for (int l = 0; l < NLF_LEVELS; ++l) EXPECT(c[l] == (float)(21.0 * NLF_K), "pooled: level %d = %g", l, c[l]);
    EXPECT(NLF_K == 4 * SIGMA_K && NLF_K == 1.0 / (1024 * 6 * 0.6744897501960817), "NLF_K");
    printf(failures ? "nlf_bounds: %d FAILURES\n" : "nlf_bounds: ok\n", failures);
    return failures != 0;
}
