// frame_finish.hip -- the output finish on the device (include/bsvd_hip.h, bsvd_blend_planar): the denoise strength, a blend of the
// network's output with its input, in place on the planar fp32 tensors between the network and the surface encoders.  A helper kernel on
// the caller's stream like those of frame_yuv.hip / frame_rgb.hip: bandwidth-bound (24 bytes read, 12 written per pixel), a grid-stride
// loop around the item body of frame_finish_items.h, which states the arithmetic and its exact ends.  Compiled without contraction
// (sources.sh).  The other half of the finish, dither, lives inside the encoders (bsvd_planar_to_*_d).
#include "bsvd_internal.h"
#include "frame_finish_items.h"

namespace bsvd {

__global__ __launch_bounds__(256) void blend_planar_kernel(float *__restrict__ y, const float *__restrict__ x, BlendGeom g, int64_t items)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x)
        blend_planar_item(y, x, g, i);
}

static int strength_check(const char *fn, const char *name, float s)
{
    if (!(s >= 0.f && s <= 1.f)) { set_error("%s: %s = %g must lie in [0, 1]", fn, name, (double)s); return -3; }   // NaN fails the comparison
    return 0;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" int bsvd_blend_planar(float *y, int64_t y_frame_stride, const float *x, int64_t x_frame_stride, int32_t frames, int32_t Hp, int32_t Wp,
                                 float s_luma, float s_chroma, const float luma_w[3], void *stream)
{
    const char *fn = "bsvd_blend_planar";
    if (!y) { set_error("%s: y is NULL", fn); return -3; }
    if (!x) { set_error("%s: x is NULL", fn); return -3; }
    if (!luma_w) { set_error("%s: luma_w is NULL", fn); return -3; }
    if (frames <= 0) { set_error("%s: frames = %d must be positive", fn, frames); return -3; }
    if (Hp <= 0) { set_error("%s: Hp = %d must be positive", fn, Hp); return -3; }
    if (Wp <= 0) { set_error("%s: Wp = %d must be positive", fn, Wp); return -3; }
    const int64_t plane = (int64_t)Hp * Wp;
    if (y_frame_stride < 3 * plane) { set_error("%s: y_frame_stride = %lld elements is below 3 planes (%lld)", fn, (long long)y_frame_stride, (long long)(3 * plane)); return -3; }
    if (x_frame_stride < 3 * plane) { set_error("%s: x_frame_stride = %lld elements is below 3 planes (%lld)", fn, (long long)x_frame_stride, (long long)(3 * plane)); return -3; }
    if (strength_check(fn, "s_luma", s_luma) || strength_check(fn, "s_chroma", s_chroma)) return -3;
    for (int c = 0; c < 3; ++c)
        if (!(luma_w[c] >= 0.f && luma_w[c] <= 1.f)) { set_error("%s: luma_w[%d] = %g must lie in [0, 1]", fn, c, (double)luma_w[c]); return -3; }
    if ((uintptr_t)y & 3) { set_error("%s: y must be 4-byte aligned", fn); return -3; }
    if ((uintptr_t)x & 3) { set_error("%s: x must be 4-byte aligned", fn); return -3; }
    BlendGeom g;
    g.y_fs = y_frame_stride; g.x_fs = x_frame_stride; g.plane = plane;
    g.vec = (Wp & 3) == 0 && aligned16(y) && aligned16(x) && (y_frame_stride & 3) == 0 && (x_frame_stride & 3) == 0;
    g.per_frame = g.vec ? plane / 4 : plane;
    g.s_c = s_chroma;
    g.om = (float)(1.0 - (double)s_chroma);
    g.dl = s_chroma - s_luma;
    for (int c = 0; c < 3; ++c) g.w[c] = luma_w[c];
    const int64_t items = g.per_frame * frames;
    return launch_sweep(blend_planar_kernel, items, stream, y, x, g, items);
}
