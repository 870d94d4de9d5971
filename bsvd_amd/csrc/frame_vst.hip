// frame_vst.hip -- the variance-stabilising transform of a noise-level curve (include/bsvd_hip.h: bsvd_vst_build, bsvd_vst_forward,
// bsvd_vst_inverse): intensities remapped so that signal-dependent noise has one standard deviation everywhere, the network's training
// condition, and mapped back afterwards.  A translation unit of its own: the code objects of the other files stay what they were.  Three
// helper kernels on the caller's stream, outside the captured graphs; the item bodies are in frame_vst_items.h.
//   build   : one workgroup of 1024 threads per curve.  Thread j computes the clamped curve at the midpoint of interval j and its double
//             reciprocal; ONE lane adds the 1024 reciprocals in ascending order (the sum's order is part of the contract, and the build
//             runs once per scene, not per frame); all threads then divide, convert and write G, R and sigma'.  Nothing crosses to the host.
//   forward : the frame's table set from device memory into LDS (G: 4 KB), planes 0 .. 2 in place, optionally one further plane filled
//             with the frame's sigma'.  blockIdx.y is the frame, so per-frame sets are one launch.
//   inverse : G and R in LDS (8 KB), the three planes of y in place.  The interval is found by ten halvings in LDS: the same ten steps in
//             every lane whatever the curve, the first steps read one address per wave (a broadcast).  A bucket index plus a walk
//             (BSVD_VST_SEARCH = 1, same bits) measured twice as fast on well-behaved curves and 3.5 x slower on a step curve, where the
//             floor packs some sixty knots into one bucket (profiles/vst.txt section 2): the bounded form is the product's.
// Built with -ffp-contract=off (sources.sh): every multiply and add of the per-pixel paths rounds separately.
#include "bsvd_internal.h"
#include "frame_vst_items.h"

#ifndef BSVD_VST_SEARCH
#define BSVD_VST_SEARCH 0            // the inverse's search: 0 the ten halvings, 1 a bucket index plus a walk; profiles/vst.txt has what both measured
#endif

namespace bsvd {

enum { VST_BLOCK = 256, VST_MAX_WGS = 2048 };

__global__ __launch_bounds__(VST_N) void vst_build_kernel(const float *__restrict__ curves, float *__restrict__ tables, float floor)
{
    __shared__ float c[NLF_LEVELS];
    __shared__ double F[VST_KNOTS];                                  // w_j first, then the running sums F_j
    __shared__ float G[VST_KNOTS];
    const int j = threadIdx.x;
    if (j < NLF_LEVELS) c[j] = curves[(int64_t)blockIdx.x * NLF_LEVELS + j];
    __syncthreads();
    F[j] = 1.0 / (double)vst_curve_value(c, j, floor);
    __syncthreads();
    if (j == 0) {
        double sum = 0.0;
#pragma unroll 8
        for (int i = 0; i < VST_N; ++i) {
            const double w = F[i];
            F[i] = sum;
            sum = sum + w;
        }
        F[VST_N] = sum;
    }
    __syncthreads();
    const double total = F[VST_N];
    float *out = tables + (int64_t)blockIdx.x * VST_TABLE_FLOATS;
    G[j] = (float)(F[j] / total);
    if (j == 0) {
        G[VST_N] = (float)(total / total);
        out[VST_SIGMA_AT] = (float)((double)VST_N / total);
        out[VST_SIGMA_AT + 1] = 0.f;
        out[VST_SIGMA_AT + 2] = 0.f;
    }
    __syncthreads();
    out[j] = G[j];
    if (j == 0) out[VST_N] = G[VST_N];
    out[VST_R_AT + j] = (float)(1.0 / ((double)G[j + 1] - (double)G[j]));
}

__global__ __launch_bounds__(VST_BLOCK) void vst_forward_kernel(float *__restrict__ x, const float *__restrict__ tables, int64_t table_stride, VstGeom g)
{
    __shared__ float G[VST_KNOTS + 1];                               // G and, behind it, sigma'
    const float *set = tables + (int64_t)blockIdx.y * table_stride;
    for (int i = threadIdx.x; i < VST_KNOTS + 1; i += VST_BLOCK) G[i] = set[i];
    __syncthreads();
    const float sigma = G[VST_SIGMA_AT];
    float *fr = x + (int64_t)blockIdx.y * g.fstride;
    for (int p = 0; p < (g.fill_plane >= 0 ? 4 : 3); ++p)
        for (int64_t i = blockIdx.x * (int64_t)VST_BLOCK + threadIdx.x; i < g.per_plane; i += (int64_t)gridDim.x * VST_BLOCK)
            vst_apply_item(fr, g, p, i, sigma, [&](float v) { return vst_forward_value(v, G); });
}

__global__ __launch_bounds__(VST_BLOCK) void vst_inverse_kernel(float *__restrict__ y, const float *__restrict__ tables, int64_t table_stride, VstGeom g)
{
    __shared__ float G[VST_KNOTS];
    __shared__ float R[VST_N];
    const float *set = tables + (int64_t)blockIdx.y * table_stride;
    for (int i = threadIdx.x; i < VST_KNOTS; i += VST_BLOCK) G[i] = set[i];
    for (int i = threadIdx.x; i < VST_N; i += VST_BLOCK) R[i] = set[VST_R_AT + i];
    __syncthreads();
    float *fr = y + (int64_t)blockIdx.y * g.fstride;
#if BSVD_VST_SEARCH == 1
    // the measured alternative: B[b] = the interval of y = b / 1024, found once per workgroup by the halvings; per element one look-up and
    // a walk up to the same k the halvings find (so the same bits), whose length depends on the curve
    __shared__ unsigned short B[VST_N];
    for (int b = threadIdx.x; b < VST_N; b += VST_BLOCK) B[b] = (unsigned short)vst_inverse_index((float)b * (1.f / VST_N), G);
    __syncthreads();
    for (int p = 0; p < 3; ++p)
        for (int64_t i = blockIdx.x * (int64_t)VST_BLOCK + threadIdx.x; i < g.per_plane; i += (int64_t)gridDim.x * VST_BLOCK)
            vst_apply_item(fr, g, p, i, 0.f, [&](float v) {
                const float t = v * (float)VST_N;
                int k = B[t >= (float)(VST_N - 1) ? VST_N - 1 : t >= 0.f ? (int)t : 0];
                while (k < VST_N - 1 && G[k + 1] <= v) ++k;
                return vst_inverse_at(v, k, G, R);
            });
#else
    for (int p = 0; p < 3; ++p)
        for (int64_t i = blockIdx.x * (int64_t)VST_BLOCK + threadIdx.x; i < g.per_plane; i += (int64_t)gridDim.x * VST_BLOCK)
            vst_apply_item(fr, g, p, i, 0.f, [&](float v) { return vst_inverse_value(v, G, R); });
#endif
}

// ---------------------------------------------------------------------------------------------
// host side: validation (no device needed), launches
static int vst_planes_check(const char *fn, const char *name, const void *x, int32_t frames, int32_t Hp, int32_t Wp, int64_t frame_stride, int planes,
                            const float *tables, int64_t table_stride)
{
    if (!x) { set_error("%s: %s is NULL", fn, name); return -3; }
    if ((uintptr_t)x & 3) { set_error("%s: %s must be 4-byte aligned", fn, name); return -3; }
    if (!tables) { set_error("%s: tables is NULL", fn); return -3; }
    if ((uintptr_t)tables & 3) { set_error("%s: tables must be 4-byte aligned", fn); return -3; }
    if (frames <= 0 || frames > 65535) { set_error("%s: frames = %d must be in 1 .. 65535", fn, frames); return -3; }
    if (Hp <= 0) { set_error("%s: Hp = %d must be positive", fn, Hp); return -3; }
    if (Wp <= 0) { set_error("%s: Wp = %d must be positive", fn, Wp); return -3; }
    const int64_t need = (int64_t)planes * Hp * Wp;
    if (frame_stride < need) {
        set_error("%s: %sframe_stride = %lld floats is below the %d planes of %d x %d it spans (%lld)", fn, name[0] == 'y' ? "y_" : "", (long long)frame_stride, planes, Hp, Wp,
                  (long long)need);
        return -3;
    }
    if (table_stride < 0 || table_stride > 65535) {
        set_error("%s: table_stride = %lld table sets must be in 0 .. 65535 (0: one table set for all frames)", fn, (long long)table_stride);
        return -3;
    }
    return 0;
}

template <class Kernel>
static int vst_launch(Kernel kernel, float *x, int32_t frames, int32_t Hp, int32_t Wp, int64_t frame_stride, int fill_plane, const float *tables,
                      int64_t table_stride, void *stream)
{
    VstGeom g;
    g.plane = (int64_t)Hp * Wp; g.fstride = frame_stride; g.fill_plane = fill_plane;
    g.vec = aligned16(x) && !(g.plane & 3) && !(frame_stride & 3);
    g.per_plane = g.vec ? g.plane / 4 : g.plane;
    unsigned gx = grid_for(g.per_plane, VST_BLOCK);
    const unsigned cap = (unsigned)VST_MAX_WGS / (unsigned)frames > 0 ? (unsigned)VST_MAX_WGS / (unsigned)frames : 1u;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)frames), dim3(VST_BLOCK), 0, (hipStream_t)stream, x, tables, table_stride * VST_TABLE_FLOATS, g);
    return (int)hipGetLastError();
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int bsvd_vst_build(const float *curves, int32_t n, float floor, float *tables, void *stream)
{
    const char *fn = "bsvd_vst_build";
    if (!curves) { set_error("%s: curves is NULL", fn); return -3; }
    if (!tables) { set_error("%s: tables is NULL", fn); return -3; }
    if (((uintptr_t)curves | (uintptr_t)tables) & 3) { set_error("%s: curves and tables must be 4-byte aligned", fn); return -3; }
    if (n <= 0 || n > 65535) { set_error("%s: n = %d must be in 1 .. 65535", fn, n); return -3; }
    if (!(floor >= 0x1p-10f && floor <= 1.f)) { set_error("%s: floor = %g must lie in [2^-10, 1]", fn, (double)floor); return -3; }   // NaN fails the comparison
    hipLaunchKernelGGL(vst_build_kernel, dim3((unsigned)n), dim3(VST_N), 0, (hipStream_t)stream, curves, tables, floor);
    return (int)hipGetLastError();
}

int bsvd_vst_forward(float *x, int32_t frames, int32_t Hp, int32_t Wp, int64_t frame_stride, int32_t fill_plane, const float *tables,
                     int64_t table_stride, void *stream)
{
    const char *fn = "bsvd_vst_forward";
    if (fill_plane >= 0 && fill_plane < 3) { set_error("%s: fill_plane = %d must be negative (no plane) or at least 3 (planes 0 .. 2 are transformed)", fn, fill_plane); return -3; }
    const int rc = vst_planes_check(fn, "x", x, frames, Hp, Wp, frame_stride, fill_plane >= 0 ? fill_plane + 1 : 3, tables, table_stride);
    if (rc) return rc;
    return vst_launch(vst_forward_kernel, x, frames, Hp, Wp, frame_stride, fill_plane >= 0 ? fill_plane : -1, tables, table_stride, stream);
}

int bsvd_vst_inverse(float *y, int64_t y_frame_stride, int32_t frames, int32_t Hp, int32_t Wp, const float *tables, int64_t table_stride, void *stream)
{
    const char *fn = "bsvd_vst_inverse";
    const int rc = vst_planes_check(fn, "y", y, frames, Hp, Wp, y_frame_stride, 3, tables, table_stride);
    if (rc) return rc;
    return vst_launch(vst_inverse_kernel, y, frames, Hp, Wp, y_frame_stride, -1, tables, table_stride, stream);
}

}  // extern "C"
