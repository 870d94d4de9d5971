// frame_sigma_items.h -- the item bodies of the noise-level estimate (include/bsvd_hip.h: bsvd_estimate_sigma, bsvd_fill_sigma_plane), as
// plain __host__ __device__ functions like those of frame_items.h / frame_surface_items.h: the kernels of frame_sigma.hip are grid-stride
// loops around them, and tools/debug/sigma_bounds.hip runs the same bodies over exact-size heap buffers under AddressSanitizer.
//
// The estimate of one frame: the Laplacian-difference mask [1 -2 1; -2 4 -2; 1 -2 1] at every interior pixel of the picture (the top-left
// H x W of each of the first `channels` planes), |r| binned into 4096 uint32 counts, the median read off the histogram, scaled by
// 1 / (6 * 0.6745).  Every step is either exact (power-of-two coefficients, integer counts) or a single correctly rounded operation in a
// fixed order, so tests/sigma_model.py reproduces the device's histogram and its sigma bit for bit.  No float sum and no float atomic
// appears anywhere: integer adds commute, which is what makes the histogram independent of the launch shape.
//
// Work shape of the histogram pass: an ITEM is 4 columns (one aligned float4 of a row) x SIGMA_BAND interior rows of one plane; consecutive
// lanes take consecutive column groups of a band, a lane walks down its band with the three stencil rows in registers, so a row is loaded
// once per band plus the two rows a band shares with its neighbours.
#pragma once
#include "frame_items.h"

namespace bsvd {

enum { SIGMA_BINS = 4096, SIGMA_BAND = 8 };
// 1 / (4096 * 6 * 0.6744897501960817): 4096 bins per unit of |r|, 6 = the mask's L2 norm, 0.6745 = the median of |N(0,1)|
constexpr double SIGMA_K = 0x1.fa0fc23747344p-15;

// H, W: the picture; Hp, Wp: the planes that hold it; ch: planes pooled; vec: rows may move as float4 (16-byte aligned base, Wp and
// fstride multiples of 4); fstride in floats
struct SigmaGeom { int H, W, Hp, Wp, ch, vec; int64_t fstride; };

BSVD_HD int sigma_groups(int W) { return (W + 2) >> 2; }                              // column groups g with an interior column: 4 g <= W - 2
BSVD_HD int sigma_bands(int H) { return (H - 2 + SIGMA_BAND - 1) / SIGMA_BAND; }
BSVD_HD int64_t sigma_items(const SigmaGeom &g) { return (int64_t)g.ch * sigma_bands(g.H) * sigma_groups(g.W); }

// columns x0 - 1 .. x0 + 4 of a row into v[0..5]; a column outside the picture's row reads as 0 and reaches no counted sample.  vec: the
// aligned float4 at x0 lies inside the row (x0 < W <= Wp, Wp a multiple of 4) even where its last columns are beyond the picture.
BSVD_HD void sigma_load_row(const float *row, int x0, int W, int vec, float *v)
{
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(row + x0);
        v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
        v[0] = x0 > 0 ? row[x0 - 1] : 0.f;
        v[5] = x0 + 4 < W ? row[x0 + 4] : 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int c = x0 - 1 + k;
            v[k] = c >= 0 && c < W ? row[c] : 0.f;
        }
    }
}

// r = (4 x_c - 2 ((x_n + x_s) + (x_w + x_e))) + ((x_nw + x_ne) + (x_sw + x_se)): the products are exact, so a contracted multiply-add
// rounds where the separate operations round
BSVD_HD float sigma_response(const float *n, const float *c, const float *s)
{
    return (4.f * c[1] - 2.f * ((n[1] + s[1]) + (c[0] + c[2]))) + ((n[0] + n[2]) + (s[0] + s[2]));
}

// q = min(floor(|r| * 4096), 4095); false: r is not finite and is not counted
BSVD_HD bool sigma_bin(float r, int *q)
{
    const float t = fabsf(r) * 4096.f;                               // exact, or +inf for a finite r beyond 2^116
    *q = t >= 4095.f ? SIGMA_BINS - 1 : t >= 0.f ? (int)t : 0;        // (NaN: bin 0, not counted)
    return fabsf(r) <= 3.402823466e+38f;                             // false for NaN and +-Inf
}

// One item of frame `x` (the frame's first element): add(q, counted) is called for each of the item's samples, counted or not -- on the
// device every lane of a wave that is in the loop reaches the call together, which is what lets it aggregate (frame_sigma.hip).
template <class Add>
BSVD_HD void sigma_hist_item(const float *x, const SigmaGeom &g, int i, Add &add)
{
    const int ng = sigma_groups(g.W), nb = sigma_bands(g.H);
    const int gi = i % ng, t = i / ng, b = t % nb, c = t / nb;
    const int x0 = gi * 4, r0 = 1 + b * SIGMA_BAND, r1 = r0 + SIGMA_BAND < g.H - 1 ? r0 + SIGMA_BAND : g.H - 1;
    const float *p = x + (int64_t)c * g.Hp * g.Wp;
    float a[6], m[6], s[6];
    sigma_load_row(p + (int64_t)(r0 - 1) * g.Wp, x0, g.W, g.vec, a);
    sigma_load_row(p + (int64_t)r0 * g.Wp, x0, g.W, g.vec, m);
    for (int r = r0; r < r1; ++r) {
        sigma_load_row(p + (int64_t)(r + 1) * g.Wp, x0, g.W, g.vec, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q;
            const bool finite = sigma_bin(sigma_response(a + k, m + k, s + k), &q);
            add(q, finite && x0 + k >= 1 && x0 + k <= g.W - 2);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) { a[k] = m[k]; m[k] = s[k]; }
    }
}

// The finish, given the median's bin: N = all counts, k = the first bin with 2 cum[k] >= N, before = cum[k] - h[k], hk = h[k] > 0.
// med = k + (N - 2 before) / (2 hk) in double; sigma = med * K * gain, clamped to [lo, hi], to fp32.  N == 0 gives lo.  No multiply feeds
// an add, so there is nothing to contract.
BSVD_HD float sigma_from_median(uint64_t N, int k, uint64_t before, uint64_t hk, float gain, float lo, float hi)
{
    if (N == 0) return lo;
    const double frac = (double)(N - 2 * before) / (double)(2 * hk);
    const double med = (double)k + frac;
    double s = med * SIGMA_K;
    s = s * (double)gain;
    if (s < (double)lo) s = (double)lo;
    if (s > (double)hi) s = (double)hi;
    return (float)s;
}

// the same from a whole histogram, serially: the host's form of the finish kernel (tools/debug/sigma_bounds.hip)
BSVD_HD float sigma_finish_serial(const uint32_t *h, float gain, float lo, float hi)
{
    uint64_t N = 0, cum = 0;
    for (int k = 0; k < SIGMA_BINS; ++k) N += h[k];
    for (int k = 0; k < SIGMA_BINS; ++k) {
        cum += h[k];
        if (N && 2 * cum >= N) return sigma_from_median(N, k, cum - h[k], h[k], gain, lo, hi);
    }
    return lo;
}

// fill: item i = elements 4 i .. 4 i + 3 of a plane of n elements
BSVD_HD void sigma_fill_item(float *plane, int64_t n, int64_t i, float v, int vec)
{
    const int64_t e = 4 * i;
    if (vec) { *reinterpret_cast<float4 *>(plane + e) = make_float4(v, v, v, v); return; }
    for (int64_t q = e; q < e + 4 && q < n; ++q) plane[q] = v;
}

}  // namespace bsvd
