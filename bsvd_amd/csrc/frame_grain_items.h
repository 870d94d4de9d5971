// frame_grain_items.h -- the item bodies of the film-grain model (include/bsvd_hip.h: bsvd_grain_stats, bsvd_grain_apply), as plain
// __host__ __device__ functions like those of frame_nlf_items.h: the kernels of frame_grain.hip are loops around them, and
// tests/grain_model.py states the same arithmetic in numpy, operation by operation.
//
// Statistics, per pixel of the picture (x the source, y the result, planes R, G, B; fp32, the translation unit is built without contraction):
//   d_c = x_c - y_c;  n0 = fmaf(w_B, d_B, fmaf(w_G, d_G, w_R * d_R)) -- the luma of the removed noise, bsvd_blend_planar's term in its order;
//   n1 = d_B - n0;  n2 = d_R - n0;  ly = fmaf(w_B, y_B, fmaf(w_G, y_G, w_R * y_R));  level l = clamp(floor(ly * 16), 0, 15), NaN: 0;
//   q_k = rintf(clamp(n_k * 4096, -2047, 2047)) as an integer; a pixel with a non-finite n_k is NOT COUNTED and all three of its q are 0.
// Everything accumulated from there on is an integer: level moments over the counted pixels, lag products over a fixed anchor set.
//
// Apply, per pixel of the whole plane, in place:
//   block (r >> 5, c >> 5) -> offsets (oy, ox) in 0 .. 96 from a hash of (seed, frame, block); g_k = tmpl_k[oy + (r & 31)][ox + (c & 31)];
//   s_k = std[k] interpolated at u = ly * 16 - 0.5 by nlf_map_value's rule; n_k = (amount * s_k) * g_k;
//   d_R = n2 + n0, d_B = n1 + n0, d_G = (n0 - (w_R * d_R + w_B * d_B)) * inv_wg; y_c += d_c.
#pragma once
#include "frame_finish_items.h"
#include "frame_nlf_items.h"

namespace bsvd {

enum {
    GRAIN_LEVELS = NLF_LEVELS,                 // 16 levels of the result's luma
    GRAIN_QMAX = 2047,                         // |q| <= 2047: a product of two is below 2^22
    GRAIN_LAG_ROWS = 3, GRAIN_LAG_COLS = 6,    // lags dy = 0 .. 3, dx = -6 .. 6
    GRAIN_LAGS = (GRAIN_LAG_COLS + 1) + GRAIN_LAG_ROWS * (2 * GRAIN_LAG_COLS + 1),       // 46
    // one frame's 256 int64: N[16], then sum q_k [3][16], then sum q_k^2 [3][16], then A[3][46], then six zeros
    GRAIN_N_AT = 0, GRAIN_S1_AT = 16, GRAIN_S2_AT = 64, GRAIN_A_AT = 112, GRAIN_STATS = 256,
    GRAIN_TMPL = 128, GRAIN_BLOCK = 32, GRAIN_OFFSETS = GRAIN_TMPL - GRAIN_BLOCK + 1      // templates 128 x 128, blocks 32 x 32, offsets 0 .. 96
};
constexpr float GRAIN_QSCALE = 4096.f;

// lag index -> (dy, dx): 0 .. 6 are dy = 0, dx = 0 .. 6; then dy = 1, 2, 3 with dx = -6 .. 6 each
BSVD_HD void grain_lag(int i, int *dy, int *dx)
{
    if (i <= GRAIN_LAG_COLS) { *dy = 0; *dx = i; return; }
    const int j = i - (GRAIN_LAG_COLS + 1);
    *dy = 1 + j / (2 * GRAIN_LAG_COLS + 1);
    *dx = j % (2 * GRAIN_LAG_COLS + 1) - GRAIN_LAG_COLS;
}

// the luma of three values, R first, then G, then B: bsvd_blend_planar's term
BSVD_HD float grain_luma(const float *w, float R, float G, float B) { return fmaf(w[2], B, fmaf(w[1], G, w[0] * R)); }

// l = clamp(floor(ly * 16), 0, 15): +inf gives 15, anything not >= 0 (NaN included) gives 0
BSVD_HD int grain_level(float ly)
{
    const float t = ly * 16.f;
    return t >= 15.f ? GRAIN_LEVELS - 1 : t >= 0.f ? (int)t : 0;
}

// One pixel: x3, y3 its R, G, B in the source and the result.  -> counted?; *l its level, q[0 .. 2] its integers (zeros when not counted).
BSVD_HD bool grain_pixel_q(const float *x3, const float *y3, const float *w, int *l, int *q)
{
    const float dR = x3[0] - y3[0], dG = x3[1] - y3[1], dB = x3[2] - y3[2];
    float n[3];
    n[0] = grain_luma(w, dR, dG, dB);
    n[1] = dB - n[0];
    n[2] = dR - n[0];
    *l = grain_level(grain_luma(w, y3[0], y3[1], y3[2]));
    bool counted = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) counted = counted && fabsf(n[k]) <= 3.402823466e+38f;     // NaN fails the comparison
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = n[k] * GRAIN_QSCALE;
        const float c = fminf(fmaxf(t, -(float)GRAIN_QMAX), (float)GRAIN_QMAX);
        q[k] = counted ? (int)rintf(c) : 0;
    }
    return counted;
}

// ---------------------------------------------------------------------------------------------
// apply

struct GrainApplyGeom {
    int Hp, Wp, vec;                        // vec: rows may move as float4 (16-byte aligned base, Wp and the frame stride multiples of 4)
    int64_t fstride, plane, per_frame;      // per_frame: the items of one frame (groups of 4 columns, or single pixels)
    float amount, w[3], inv_wg;
    uint32_t seed;
    int64_t frame0;
    float std[3][GRAIN_LEVELS];
};

// the (seed, frame) part of a block's hash: the dither's key with component 3, which no dither uses
BSVD_HD uint32_t grain_frame_key(uint32_t seed, int64_t frame) { return dither_frame_key(seed, frame, 3); }

// block (by, bx) -> its offsets into the templates, each in 0 .. 96: the two 16-bit halves of the hash, scaled by 97 / 65536
BSVD_HD void grain_block_offsets(uint32_t kf, int by, int bx, int *oy, int *ox)
{
    const uint32_t h = fmix32(kf ^ ((uint32_t)bx + (uint32_t)by * 0x9e3779b1u));
    *oy = (int)(((h >> 16) * (uint32_t)GRAIN_OFFSETS) >> 16);
    *ox = (int)(((h & 0xffffu) * (uint32_t)GRAIN_OFFSETS) >> 16);
}

// std[k] interpolated between the level centres at u = ly * 16 - 0.5: nlf_map_value's rule from u on
BSVD_HD void grain_scale(float ly, const float (*std)[GRAIN_LEVELS], float *s)
{
    float u = ly * 16.f - 0.5f;
    u = u >= 15.f ? 15.f : u >= 0.f ? u : 0.f;
    int i = (int)u;
    if (i > GRAIN_LEVELS - 2) i = GRAIN_LEVELS - 2;
    const float f = u - (float)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = std[k][i + 1] - std[k][i];
        const float fd = f * d;
        s[k] = std[k][i] + fd;
    }
}

// one pixel: y3 its R, G, B, g3 the three templates' samples
BSVD_HD void grain_apply_pixel(const GrainApplyGeom &g, const float (*std)[GRAIN_LEVELS], float *y3, const float *g3)
{
    float s[3], n[3];
    grain_scale(grain_luma(g.w, y3[0], y3[1], y3[2]), std, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = g.amount * s[k];
        n[k] = a * g3[k];
    }
    const float dR = n[2] + n[0], dB = n[1] + n[0];
    const float pr = g.w[0] * dR, pb = g.w[2] * dB;
    const float t = pr + pb;
    const float dG = (n[0] - t) * g.inv_wg;
    y3[0] = y3[0] + dR;
    y3[1] = y3[1] + dG;
    y3[2] = y3[2] + dB;
}

// One item of frame f (the call's index; its stream index is frame0 + f): 4 consecutive columns of one row (vec) or one pixel.  An aligned
// group of 4 columns lies in one block.  tmpl: [3][128][128]; std: g.std or a copy of it (the kernel's is in LDS: the level index differs per lane).
BSVD_HD void grain_apply_item(float *y, const float *tmpl, const GrainApplyGeom &g, const float (*std)[GRAIN_LEVELS], int64_t i)
{
    const int64_t f = i / g.per_frame, e = (i - f * g.per_frame) * (g.vec ? 4 : 1);
    const int r = (int)(e / g.Wp), c = (int)(e - (int64_t)r * g.Wp);
    int oy, ox;
    grain_block_offsets(grain_frame_key(g.seed, g.frame0 + f), r >> 5, c >> 5, &oy, &ox);
    const float *t0 = tmpl + (oy + (r & 31)) * GRAIN_TMPL + ox + (c & 31);
    float *yp = y + f * g.fstride + e;
    if (g.vec) {
        float4 yv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) yv[k] = *reinterpret_cast<const float4 *>(yp + k * g.plane);
        float a[4][3], t[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[0][k] = yv[k].x; a[1][k] = yv[k].y; a[2][k] = yv[k].z; a[3][k] = yv[k].w;
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q][k] = t0[k * GRAIN_TMPL * GRAIN_TMPL + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) grain_apply_pixel(g, std, a[q], t[q]);
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<float4 *>(yp + k * g.plane) = make_float4(a[0][k], a[1][k], a[2][k], a[3][k]);
    } else {
        float a[3] = {yp[0], yp[g.plane], yp[2 * g.plane]};
        const float t[3] = {t0[0], t0[GRAIN_TMPL * GRAIN_TMPL], t0[2 * GRAIN_TMPL * GRAIN_TMPL]};
        grain_apply_pixel(g, std, a, t);
        yp[0] = a[0]; yp[g.plane] = a[1]; yp[2 * g.plane] = a[2];
    }
}

}  // namespace bsvd
