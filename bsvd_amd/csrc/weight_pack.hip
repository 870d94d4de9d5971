// weight_pack.hip -- weight pre-pack (include/bsvd_hip.h: bsvd_pack_weights, bsvd_pack_weights_wino, bsvd_pack_head_weights and the
// bsvd_packed_* sizes): one-time transforms of nn.Conv2d weights into the layouts the conv kernels stream, run once per model load.
#include <math.h>
#include "bsvd_internal.h"
#include "wino_forms.h"

namespace bsvd {

// what every pack sweep reads: the OIHW fp32 source, its real and padded sizes, the bias pair (both nullable)
struct PackSrc { const float *w, *bias; int Cin, Cout, Cin_pad, Cout_pad, ps; float *bp; };

// Packed output channel np -> its source channel *n; false = a pad channel.  A PixelShuffle layer (ps) is packed sub-pixel major -- packed
// channel np = [4 sub-pixels][Cout_pad / 4] <- source channel 4 ch + sub -- so that the 8 channels a lane stores land in one output pixel.
__device__ __forceinline__ bool pack_channel(int np, int ps, int Cout, int Cout_pad, int *n)
{
    if (!ps) { *n = np; return np < Cout; }
    const int Cq_pad = Cout_pad >> 2, sub = np / Cq_pad, ch = np - sub * Cq_pad;
    *n = 4 * ch + sub;
    return ch < (Cout >> 2);
}

// the 9 taps of (packed output channel np, input channel c) in the source, nullptr where the pack holds zeros (a pad channel on either side)
__device__ __forceinline__ const float *pack_taps(const PackSrc &s, int np, int c)
{
    int n;
    const bool ok = pack_channel(np, s.ps, s.Cout, s.Cout_pad, &n);
    return ok && c < s.Cin ? s.w + ((int64_t)n * s.Cin + c) * 9 : nullptr;
}

// The bias in packed channel order: the first Cout_pad items of every pack sweep write it.
__device__ __forceinline__ void pack_bias(int64_t i, const PackSrc &s)
{
    if (!s.bp || i >= s.Cout_pad) return;
    int n;
    const bool ok = pack_channel((int)i, s.ps, s.Cout, s.Cout_pad, &n);
    s.bp[i] = (ok && s.bias) ? s.bias[n] : 0.f;
}

// OIHW fp32 -> [Cin_pad/16][9][4][Cout_pad][4]
__global__ void pack_weights_kernel(PackSrc s, float *__restrict__ wp)
{
    const int64_t total = (int64_t)s.Cin_pad * 9 * s.Cout_pad;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int j = t & 3; t >>= 2;
        const int np = (int)(t % s.Cout_pad); t /= s.Cout_pad;
        const int k4 = t & 3; t >>= 2;
        const int tap = (int)(t % 9), cb = (int)(t / 9);
        const float *g = pack_taps(s, np, cb * 16 + k4 * 4 + j);
        wp[i] = g ? g[tap] : 0.f;
        pack_bias(i, s);
    }
}

// The fp16-pair packs, [Cin_pad/16][R rows][part: hi, lo][h = 2][Cout_pad][8 fp16]: element (h, j) is input channel 8h + j of the chunk -- the
// k-slot lane (n, h) of v_mfma_f32_32x32x16_f16 feeds.  R = 9 taps of the direct form (same byte size as the fp32 pack), A x 3 (xi, ky)
// of the Winograd form.
struct PairItem { int np, c, row, part; };
__device__ __forceinline__ PairItem pair_item(int64_t t, int Cout_pad, int rows)
{
    PairItem it;
    const int j = t & 7; t >>= 3;
    it.np = (int)(t % Cout_pad); t /= Cout_pad;
    const int h = t & 1; t >>= 1;
    it.part = t & 1; t >>= 1;
    it.row = (int)(t % rows);
    it.c = (int)(t / rows) * 16 + h * 8 + j;
    return it;
}

__global__ void pack_weights_split_kernel(PackSrc s, _Float16 *__restrict__ wp)
{
    const int64_t total = (int64_t)s.Cin_pad * 9 * s.Cout_pad * 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const PairItem it = pair_item(i, s.Cout_pad, 9);
        const float *g = pack_taps(s, it.np, it.c);
        float v = g ? g[it.row] : 0.f;
        v = fminf(fmaxf(v, -65504.f), 65504.f);        // fp16 range: saturate, never an (inf, NaN) pair (hosts refuse such weights first)
        const _Float16 hi = (_Float16)v;
        wp[i] = it.part ? (_Float16)(v - (float)hi) : hi;
        pack_bias(i, s);
    }
}

// Winograd weights (conv3x3_winox.hip): rows = [A][3 ky], U = G g along kx in double
struct WinoG { double g[8][3]; int a; };
template <int M> static WinoG wino_g()
{
    WinoG G = {};
    G.a = M + 2;
    for (int i = 0; i < 3 * (M + 2); ++i) G.g[i / 3][i % 3] = WinoForm<M>::G[i / 3][i % 3];
    return G;
}

__global__ void pack_weights_wino_kernel(PackSrc s, WinoG G, _Float16 *__restrict__ wp)
{
    const int64_t total = (int64_t)s.Cin_pad * 3 * G.a * s.Cout_pad * 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const PairItem it = pair_item(i, s.Cout_pad, 3 * G.a);
        const int xi = it.row / 3, ky = it.row - 3 * xi;
        double u = 0.0;
        if (const float *g = pack_taps(s, it.np, it.c)) {
            g += ky * 3;
            u = G.g[xi][0] * (double)g[0] + G.g[xi][1] * (double)g[1] + G.g[xi][2] * (double)g[2];
        }
        // fp16 range: U = G g reaches 1.5x (F(2,3)) .. 15x (F(6,3)) the largest weight.  Saturate instead of packing (inf, NaN); hosts keep
        // such a layer on the direct form (engine.PackedNet tests max |w| x the form's largest |G| row sum against fp16's range)
        u = u > 65504.0 ? 65504.0 : (u < -65504.0 ? -65504.0 : u);
        const _Float16 hi = (_Float16)u;
        wp[i] = it.part ? (_Float16)(u - (double)hi) : hi;
        pack_bias(i, s);
    }
}

// weights of the fused network entry: one thread per (pair, k-step, lane, j): A operand of v_mfma_f32_32x32x16_f16, rows = the
// channel permutation `chan` of conv3x3_kernel (a lane ends with two groups of 8 consecutive channels)
__global__ void pack_head_weights_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin, int Cmid, int Cmid_pad, _Float16 *__restrict__ wp, float *__restrict__ bp)
{
    const int total = (Cmid_pad / 32) * 3 * 64 * 8;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i & 7, lane = (i >> 3) & 63, ps = i >> 9, sidx = ps % 3, pair = ps / 3;
        const int row = lane & 31, kb = lane >> 5;
        const int rrow = (row & 3) + 4 * (row >> 3);
        const int ch = pair * 32 + 8 * (2 * (rrow >> 3) + ((row >> 2) & 1)) + (rrow & 7);
        const int k = 16 * sidx + 8 * kb + j, tap = k >> 2, c = k & 3;
        float v = 0.f;
        if (ch < Cmid && tap < 9 && c < Cin) v = w[((int64_t)ch * Cin + c) * 9 + tap];
        v = fminf(fmaxf(v, -65504.f), 65504.f);
        const _Float16 hi = (_Float16)v;
        _Float16 *dst = wp + ((int64_t)(ps * 64 + lane)) * 16;
        dst[j] = hi;
        dst[8 + j] = (_Float16)(v - (float)hi);
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Cmid_pad; i += gridDim.x * blockDim.x)
        bp[i] = (bias && i < Cmid) ? bias[i] : 0.f;
}

// the size checks of bsvd_pack_weights (Cout_pad % 16) and bsvd_pack_weights_wino (Cout_pad % 32, and says so)
static int pack_check(const char *fn, const PackSrc &s, const void *wp, int cout_align)
{
    if (!s.w || !wp) { set_error("%s: NULL weight pointer", fn); return -3; }
    if (s.Cin <= 0 || s.Cout <= 0 || s.Cin_pad < s.Cin || s.Cout_pad < s.Cout || (s.Cin_pad & 15) || (s.Cout_pad & (cout_align - 1))) {
        set_error("%s: bad sizes Cin %d->%d Cout %d->%d%s", fn, s.Cin, s.Cin_pad, s.Cout, s.Cout_pad, cout_align == 32 ? " (Cin_pad % 16, Cout_pad % 32)" : "");
        return -5;
    }
    if (s.ps && ((s.Cout & 3) || (s.Cout_pad & 63))) { set_error("%s: pixel_shuffle needs Cout %% 4 == 0 and Cout_pad %% 64 == 0", fn); return -10; }
    return 0;
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int64_t bsvd_packed_weight_elems(int32_t Cin_pad, int32_t Cout_pad) { return (int64_t)Cin_pad * 9 * Cout_pad; }
int64_t bsvd_packed_wino_weight_elems(int32_t Cin_pad, int32_t Cout_pad, int32_t m) { return (int64_t)Cin_pad * 3 * (m + 2) * Cout_pad; }
int64_t bsvd_packed_head_weight_bytes(int32_t Cmid_pad) { return (int64_t)(Cmid_pad / 32) * 3 * 64 * 32; }

int bsvd_pack_weights(const float *w, const float *bias, int32_t Cin, int32_t Cout, int32_t Cin_pad, int32_t Cout_pad, int32_t pixel_shuffle, int32_t dtype, void *wp, void *bp, void *stream)
{
    if (dtype != BSVD_F32 && dtype != BSVD_F16X3) { set_error("bsvd_pack_weights: dtype %d not supported", dtype); return -2; }
    const PackSrc s = {w, bias, Cin, Cout, Cin_pad, Cout_pad, pixel_shuffle ? 1 : 0, (float *)bp};
    if (const int rc = pack_check("bsvd_pack_weights", s, wp, 16)) return rc;
    const int64_t total = bsvd_packed_weight_elems(Cin_pad, Cout_pad);
    if (dtype == BSVD_F16X3) return launch_sweep(pack_weights_split_kernel, 2 * total, stream, s, (_Float16 *)wp);
    return launch_sweep(pack_weights_kernel, total, stream, s, (float *)wp);
}

int bsvd_pack_weights_wino(const float *w, const float *bias, int32_t Cin, int32_t Cout, int32_t Cin_pad, int32_t Cout_pad, int32_t pixel_shuffle, int32_t m, void *wp, void *bp, void *stream)
{
    if (!wino_m_ok(m)) { set_error("bsvd_pack_weights_wino: m = %d (2, 4 or 6)", m); return -2; }
    const PackSrc s = {w, bias, Cin, Cout, Cin_pad, Cout_pad, pixel_shuffle ? 1 : 0, (float *)bp};
    if (const int rc = pack_check("bsvd_pack_weights_wino", s, wp, 32)) return rc;
    const WinoG G = m == 2 ? wino_g<2>() : m == 4 ? wino_g<4>() : wino_g<6>();
    return launch_sweep(pack_weights_wino_kernel, 2 * bsvd_packed_wino_weight_elems(Cin_pad, Cout_pad, m), stream, s, G, (_Float16 *)wp);
}

int bsvd_pack_head_weights(const float *w, const float *bias, int32_t Cin, int32_t Cmid, int32_t Cmid_pad, void *wp, float *bp, void *stream)
{
    if (!w || !wp || !bp) { set_error("bsvd_pack_head_weights: NULL pointer"); return -3; }
    if ((Cin != 3 && Cin != 4) || Cmid <= 0 || Cmid_pad < Cmid || (Cmid_pad & 31)) { set_error("bsvd_pack_head_weights: needs Cin 3|4 and Cmid_pad %% 32 == 0 (Cin %d, Cmid %d -> %d)", Cin, Cmid, Cmid_pad); return -5; }
    return launch_sweep(pack_head_weights_kernel, (int64_t)(Cmid_pad / 32) * 3 * 64 * 8, stream, w, bias, Cin, Cmid, Cmid_pad, (_Float16 *)wp, bp);
}

}  // extern "C"
