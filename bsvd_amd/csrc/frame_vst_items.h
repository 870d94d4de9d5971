// frame_vst_items.h -- the item bodies of the variance-stabilising transform (include/bsvd_hip.h: bsvd_vst_build, bsvd_vst_forward,
// bsvd_vst_inverse), as plain __host__ __device__ functions like those of frame_nlf_items.h: the kernels of frame_vst.hip are loops
// around them.
//
// One table set per noise curve: with N = 1024 intervals over [0, 1], G[0 .. N] (the transform at the knots j / N, G[0] = 0, G[N] = 1),
// R[0 .. N - 1] (the reciprocal of each interval's rise) and sigma' (the one standard deviation the noise has after the transform).
// Layout of a set, VST_TABLE_FLOATS floats: G at 0, sigma' at VST_SIGMA_AT, two zeros, R at VST_R_AT (a multiple of 4).
// The build is in double, ascending, every operation rounded once; the per-pixel paths multiply, add and compare in fp32, every operation
// rounded separately (the translation unit is built without contraction): tests/vst_model.py reproduces all three bit for bit.
#pragma once
#include "frame_nlf_items.h"

namespace bsvd {

enum { VST_N = 1024, VST_KNOTS = VST_N + 1, VST_SIGMA_AT = VST_KNOTS, VST_R_AT = VST_KNOTS + 3, VST_TABLE_FLOATS = VST_R_AT + VST_N };

// s_j: the curve at the midpoint of interval j, bsvd_fill_nlf_plane's interpolation rule, clamped to [floor, 1] (not-a-number: floor)
BSVD_HD float vst_curve_value(const float *c, int j, float floor)
{
    float u = ((float)j + 0.5f) * (16.f / VST_N) - 0.5f;               // exact in fp32
    u = u >= 15.f ? 15.f : u >= 0.f ? u : 0.f;
    int i = (int)u;
    if (i > NLF_LEVELS - 2) i = NLF_LEVELS - 2;
    const float f = u - (float)i;
    const float d = c[i + 1] - c[i];
    const float fd = f * d;
    float s = c[i] + fd;
    s = s >= floor ? s : floor;
    return s <= 1.f ? s : 1.f;
}

// y = G[k] + fr * (G[k+1] - G[k]) with k = clamp((int)(x * 1024), 0, 1023) (NaN: 0), fr = x * 1024 - k: values outside [0, 1] continue on
// the end interval's line
BSVD_HD float vst_forward_value(float x, const float *G)
{
    const float t = x * (float)VST_N;
    const int k = t >= (float)(VST_N - 1) ? VST_N - 1 : t >= 0.f ? (int)t : 0;
    const float fr = t - (float)k;
    const float g0 = G[k];
    const float d = G[k + 1] - g0;
    const float fd = fr * d;
    return g0 + fd;
}

// k = the largest index in 0 .. 1023 with G[k] <= y (0 if there is none; NaN: 0), by ten halvings: every lane does the same ten steps;
// x = ((float)k + (y - G[k]) * R[k]) / 1024
BSVD_HD int vst_inverse_index(float y, const float *G)
{
    int k = 0;
#pragma unroll
    for (int step = VST_N / 2; step >= 1; step >>= 1)
        if (G[k + step] <= y) k += step;
    return k;
}

BSVD_HD float vst_inverse_at(float y, int k, const float *G, const float *R)
{
    const float d = y - G[k];
    const float p = d * R[k];
    const float s = (float)k + p;
    return s * (1.f / VST_N);
}

BSVD_HD float vst_inverse_value(float y, const float *G, const float *R) { return vst_inverse_at(y, vst_inverse_index(y, G), G, R); }

// planes of one frame as one run of floats per plane (rows are Wp apart and tight); vec: a plane may move as float4 (16-byte aligned
// base, Hp * Wp and the frame stride multiples of 4).  fill_plane < 0: no plane is filled.
// per_plane: the items of one plane (float4s or floats); an item is (p, off): p = 0 .. 2 a colour plane, p = 3 the filled plane.
struct VstGeom { int64_t plane, fstride, per_plane; int fill_plane, vec; };

template <class Fn>
BSVD_HD void vst_apply_item(float *fr, const VstGeom &g, int p, int64_t off, float sigma, Fn fn)
{
    if (p < 3) {
        float *at = fr + p * g.plane;
        if (g.vec) {
            float4 v = reinterpret_cast<float4 *>(at)[off];
            v.x = fn(v.x); v.y = fn(v.y); v.z = fn(v.z); v.w = fn(v.w);
            reinterpret_cast<float4 *>(at)[off] = v;
        } else {
            at[off] = fn(at[off]);
        }
    } else {
        float *at = fr + (int64_t)g.fill_plane * g.plane;
        if (g.vec) reinterpret_cast<float4 *>(at)[off] = make_float4(sigma, sigma, sigma, sigma);
        else at[off] = sigma;
    }
}

}  // namespace bsvd
