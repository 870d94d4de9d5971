// frame_nlf_items.h -- the item bodies of the noise-level function (include/bsvd_hip.h: bsvd_estimate_nlf, bsvd_fill_nlf_plane), as plain
// __host__ __device__ functions like those of frame_sigma_items.h: the kernels of frame_nlf.hip are grid-stride loops around them, and
// tools/debug/nlf_bounds.hip runs the same bodies over exact-size heap buffers under AddressSanitizer.
//
// One frame: the sample of frame_sigma_items.h (the Laplacian-difference response r at every interior pixel of the picture in the three
// colour planes), keyed by the 3 x 3 box sum S of the same nine values: level l = clamp(floor(S * 16/9), 0, 15), bin q = min(floor(|r| *
// 1024), 1023), uint32 counts [16][1024].  The curve: per level the median bin, / (1024 * 6 * 0.6745); a level below min_count samples takes
// the nearest valid level's value.  The map: at every pixel of the whole plane the box sums of the three planes (replicate border), their
// 1:2:1 mix as a position u on the level axis, the curve interpolated between level centres.  Every step is exact, an integer count, or one
// correctly rounded operation in a fixed order: tests/nlf_model.py reproduces histogram, curve and map bit for bit.
//
// Work shape of both passes: an ITEM is 4 columns (one aligned float4 of a row) x NLF_BAND rows; a lane walks down its band with the three
// stencil rows in registers, so a row is loaded once per band plus the two rows a band shares with its neighbours.
#pragma once
#include "frame_sigma_items.h"

namespace bsvd {

enum { NLF_LEVELS = 16, NLF_BINS = 1024, NLF_BAND = SIGMA_BAND, NLF_HIST = NLF_LEVELS * NLF_BINS };
// 1 / (1024 * 6 * 0.6744897501960817) = 4 SIGMA_K
constexpr double NLF_K = 0x1.fa0fc23747344p-13;
constexpr float NLF_LEVEL_SCALE = (float)(16.0 / 9.0);               // box sum of one plane -> level axis
constexpr float NLF_MAP_SCALE = (float)(16.0 / 36.0);                // (S_R + S_B) + 2 S_G -> level axis

// the horizontal part of the box sum: (x_w + x_c) + x_e
BSVD_HD float nlf_row_sum(const float *v) { return (v[0] + v[1]) + v[2]; }
// S = (row_n + row_c) + row_s
BSVD_HD float nlf_box_sum(const float *n, const float *c, const float *s) { return (nlf_row_sum(n) + nlf_row_sum(c)) + nlf_row_sum(s); }

// l = clamp(floor(S * 16/9), 0, 15): +inf gives 15, anything not >= 0 (NaN included) gives 0
BSVD_HD int nlf_level(float S)
{
    const float t = S * NLF_LEVEL_SCALE;
    return t >= 15.f ? NLF_LEVELS - 1 : t >= 0.f ? (int)t : 0;
}

// q = min(floor(|r| * 1024), 1023); false: r is not finite and is not counted (the rule of sigma_bin)
BSVD_HD bool nlf_bin(float r, int *q)
{
    const float t = fabsf(r) * 1024.f;
    *q = t >= 1023.f ? NLF_BINS - 1 : t >= 0.f ? (int)t : 0;
    return fabsf(r) <= 3.402823466e+38f;
}

// One item of frame `x`: add(key, counted) with key = (l << 10) | q for each of the item's samples, counted or not (every lane of a wave
// that is in the loop reaches the call together, frame_nlf.hip).  g.ch planes are sampled (3 for the ABI).
template <class Add>
BSVD_HD void nlf_hist_item(const float *x, const SigmaGeom &g, int i, Add &add)
{
    const int ng = sigma_groups(g.W), nb = sigma_bands(g.H);
    const int gi = i % ng, t = i / ng, b = t % nb, c = t / nb;
    const int x0 = gi * 4, r0 = 1 + b * NLF_BAND, r1 = r0 + NLF_BAND < g.H - 1 ? r0 + NLF_BAND : g.H - 1;
    const float *p = x + (int64_t)c * g.Hp * g.Wp;
    float a[6], m[6], s[6];
    sigma_load_row(p + (int64_t)(r0 - 1) * g.Wp, x0, g.W, g.vec, a);
    sigma_load_row(p + (int64_t)r0 * g.Wp, x0, g.W, g.vec, m);
    for (int r = r0; r < r1; ++r) {
        sigma_load_row(p + (int64_t)(r + 1) * g.Wp, x0, g.W, g.vec, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q;
            const bool finite = nlf_bin(sigma_response(a + k, m + k, s + k), &q);
            const int l = nlf_level(nlf_box_sum(a + k, m + k, s + k));
            add((l << 10) | q, finite && x0 + k >= 1 && x0 + k <= g.W - 2);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) { a[k] = m[k]; m[k] = s[k]; }
    }
}

// The value of one level (or of the pooled histogram), given the median's bin: sigma_from_median with 1024 bins per unit of |r|
BSVD_HD float nlf_from_median(uint64_t N, int k, uint64_t before, uint64_t hk, float gain, float lo, float hi)
{
    if (N == 0) return lo;
    const double frac = (double)(N - 2 * before) / (double)(2 * hk);
    const double med = (double)k + frac;
    double s = med * NLF_K;
    s = s * (double)gain;
    if (s < (double)lo) s = (double)lo;
    if (s > (double)hi) s = (double)hi;
    return (float)s;
}

// the fill of the levels that are not valid: the nearest valid level's value, the lower level on a tie; no valid level: the pooled value
BSVD_HD float nlf_level_value(int l, const float *own, unsigned valid_mask, float pooled)
{
    if (!valid_mask) return pooled;
    for (int d = 0; d < NLF_LEVELS; ++d) {
        if (l - d >= 0 && (valid_mask >> (l - d) & 1)) return own[l - d];
        if (l + d < NLF_LEVELS && (valid_mask >> (l + d) & 1)) return own[l + d];
    }
    return pooled;
}

// the value of the first `levels` histograms at h, summed bin by bin, serially; *N_out: their samples
BSVD_HD float nlf_median_serial(const uint32_t *h, int levels, float gain, float lo, float hi, uint64_t *N_out)
{
    uint64_t N = 0, cum = 0;
    for (int k = 0; k < NLF_BINS; ++k)
        for (int l = 0; l < levels; ++l) N += h[l * NLF_BINS + k];
    *N_out = N;
    for (int k = 0; k < NLF_BINS; ++k) {
        uint64_t hk = 0;
        for (int l = 0; l < levels; ++l) hk += h[l * NLF_BINS + k];
        cum += hk;
        if (N && 2 * cum >= N) return nlf_from_median(N, k, cum - hk, hk, gain, lo, hi);
    }
    return lo;
}

// the whole finish of one frame, serially: the host's form of the finish kernel (tools/debug/nlf_bounds.hip)
BSVD_HD void nlf_finish_serial(const uint32_t *h, float gain, float lo, float hi, int min_count, float *curve)
{
    float own[NLF_LEVELS];
    unsigned valid = 0;
    uint64_t N;
    for (int l = 0; l < NLF_LEVELS; ++l) {
        own[l] = nlf_median_serial(h + l * NLF_BINS, 1, gain, lo, hi, &N);
        if (N >= (uint64_t)min_count) valid |= 1u << l;
    }
    const float pooled = nlf_median_serial(h, NLF_LEVELS, gain, lo, hi, &N);
    for (int l = 0; l < NLF_LEVELS; ++l) curve[l] = nlf_level_value(l, own, valid, pooled);
}

// ---------------------------------------------------------------------------------------------
// the map: planes 0 .. 2 of a frame through the box stencil with replicate borders, plane `out_plane` written

// Hp, Wp: the planes; vec: rows may move as float4 (16-byte aligned base, Wp and the frame stride multiples of 4)
struct NlfMapGeom { int Hp, Wp, out_plane, vec; int64_t fstride; };

BSVD_HD int nlf_map_groups(int Wp) { return (Wp + 3) >> 2; }
BSVD_HD int nlf_map_bands(int Hp) { return (Hp + NLF_BAND - 1) / NLF_BAND; }
BSVD_HD int64_t nlf_map_items(const NlfMapGeom &g) { return (int64_t)nlf_map_bands(g.Hp) * nlf_map_groups(g.Wp); }

// the four horizontal sums of row `r` (clamped to the plane) at columns x0 .. x0 + 3, columns clamped to the plane
BSVD_HD void nlf_map_row(const float *plane, int r, int x0, int Hp, int Wp, int vec, float *h)
{
    const float *row = plane + (int64_t)(r < 0 ? 0 : r > Hp - 1 ? Hp - 1 : r) * Wp;
    float v[6];
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(row + x0);
        v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
        v[0] = row[x0 > 0 ? x0 - 1 : 0];
        v[5] = row[x0 + 4 < Wp ? x0 + 4 : Wp - 1];
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int c = x0 - 1 + k;
            v[k] = row[c < 0 ? 0 : c > Wp - 1 ? Wp - 1 : c];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = nlf_row_sum(v + k);
}

// u = ((S_R + S_B) + 2 S_G) * (16/36) - 0.5 clamped to [0, 15] (NaN: 0); i = min((int)u, 14), f = u - i; c[i] + f * (c[i+1] - c[i]).
// The multiply and the add round separately: the translation unit is built without contraction.
BSVD_HD float nlf_map_value(float SR, float SG, float SB, const float *curve)
{
    const float mix = (SR + SB) + 2.f * SG;
    float u = mix * NLF_MAP_SCALE - 0.5f;
    u = u >= 15.f ? 15.f : u >= 0.f ? u : 0.f;
    int i = (int)u;
    if (i > NLF_LEVELS - 2) i = NLF_LEVELS - 2;
    const float f = u - (float)i;
    const float d = curve[i + 1] - curve[i];
    const float fd = f * d;
    return curve[i] + fd;
}

// One item of frame `x`: columns 4 gi .. 4 gi + 3 of rows b NLF_BAND .. of the map plane
BSVD_HD void nlf_map_item(float *x, const NlfMapGeom &g, const float *curve, int64_t i)
{
    const int ng = nlf_map_groups(g.Wp);
    const int gi = (int)(i % ng), b = (int)(i / ng);
    const int x0 = gi * 4, r0 = b * NLF_BAND, r1 = r0 + NLF_BAND < g.Hp ? r0 + NLF_BAND : g.Hp;
    const int64_t plane = (int64_t)g.Hp * g.Wp;
    float a[3][4], m[3][4], s[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        nlf_map_row(x + c * plane, r0 - 1, x0, g.Hp, g.Wp, g.vec, a[c]);
        nlf_map_row(x + c * plane, r0, x0, g.Hp, g.Wp, g.vec, m[c]);
    }
    float *out = x + (int64_t)g.out_plane * plane;
    for (int r = r0; r < r1; ++r) {
        float S[3][4], v[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nlf_map_row(x + c * plane, r + 1, x0, g.Hp, g.Wp, g.vec, s[c]);
#pragma unroll
            for (int k = 0; k < 4; ++k) { S[c][k] = (a[c][k] + m[c][k]) + s[c][k]; a[c][k] = m[c][k]; m[c][k] = s[c][k]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = nlf_map_value(S[0][k], S[1][k], S[2][k], curve);
        float *at = out + (int64_t)r * g.Wp + x0;
        if (g.vec) *reinterpret_cast<float4 *>(at) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int k = 0; k < 4 && x0 + k < g.Wp; ++k) at[k] = v[k];
    }
}

}  // namespace bsvd
