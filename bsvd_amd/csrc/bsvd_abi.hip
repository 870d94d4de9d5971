// bsvd_abi.hip -- C-ABI entry points of libbsvd_hip.so (see include/bsvd_hip.h): argument validation,
// dispatch, and the small bandwidth-bound helper kernels (weight pre-pack, NCHW<->NHWC, halo pack).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "bsvd_internal.h"
#include "wino_forms.h"

namespace bsvd {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------------------------------------
// weight pre-pack.  A PixelShuffle layer (ps) is packed sub-pixel major -- packed channel np = [4 sub-pixels][Cout_pad / 4] <- source
// channel 4 ch + sub -- so that the 8 channels a lane stores land in one output pixel.
// The bias in that channel order: the first Cout_pad elements of every pack kernel's sweep write it.
__device__ __forceinline__ void pack_bias(int64_t i, const float *__restrict__ bias, int ps, int Cout, int Cout_pad, float *__restrict__ bp)
{
    const int Cq_pad = Cout_pad >> 2, Cq = Cout >> 2;
    if (bp && i < Cout_pad) {
        int nb = (int)i;
        bool okb;
        if (ps) {
            const int sub = nb / Cq_pad, ch = nb - sub * Cq_pad;
            okb = ch < Cq;
            nb = 4 * ch + sub;
        } else {
            okb = nb < Cout;
        }
        bp[i] = (okb && bias) ? bias[nb] : 0.f;
    }
}

// OIHW fp32 -> [Cin_pad/16][9][4][Cout_pad][4]
__global__ void pack_weights_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin, int Cout,
                                    int Cin_pad, int Cout_pad, int ps, float *__restrict__ wp,
                                    float *__restrict__ bp)
{
    const int64_t total = (int64_t)Cin_pad * 9 * Cout_pad;
    const int Cq_pad = Cout_pad >> 2, Cq = Cout >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int j = t & 3; t >>= 2;
        const int np = (int)(t % Cout_pad); t /= Cout_pad;
        const int k4 = t & 3; t >>= 2;
        const int tap = (int)(t % 9);
        const int cb = (int)(t / 9);
        const int c = cb * 16 + k4 * 4 + j;
        int n = np;
        bool ok = c < Cin;
        if (ps) {
            const int sub = np / Cq_pad, ch = np - sub * Cq_pad;
            ok = ok && ch < Cq;
            n = 4 * ch + sub;
        } else {
            ok = ok && np < Cout;
        }
        wp[i] = ok ? w[((int64_t)n * Cin + c) * 9 + tap] : 0.f;
        pack_bias(i, bias, ps, Cout, Cout_pad, bp);
    }
}

// split16 weights: [Cin_pad/16][9][part: hi, lo][h = 2][Cout_pad][8 fp16]; element (h, j) is input channel 8h + j of the
// chunk -- the k-slot lane (n, h) of v_mfma_f32_32x32x16_f16 feeds.  Same byte size as the fp32 pack.
__global__ void pack_weights_split_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin, int Cout,
                                          int Cin_pad, int Cout_pad, int ps, _Float16 *__restrict__ wp,
                                          float *__restrict__ bp)
{
    const int64_t total = (int64_t)Cin_pad * 9 * Cout_pad * 2;
    const int Cq_pad = Cout_pad >> 2, Cq = Cout >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int j = t & 7; t >>= 3;
        const int np = (int)(t % Cout_pad); t /= Cout_pad;
        const int h = t & 1; t >>= 1;
        const int part = t & 1; t >>= 1;
        const int tap = (int)(t % 9);
        const int cb = (int)(t / 9);
        const int c = cb * 16 + h * 8 + j;
        int n = np;
        bool ok = c < Cin;
        if (ps) {
            const int sub = np / Cq_pad, ch = np - sub * Cq_pad;
            ok = ok && ch < Cq;
            n = 4 * ch + sub;
        } else {
            ok = ok && np < Cout;
        }
        float v = ok ? w[((int64_t)n * Cin + c) * 9 + tap] : 0.f;
        v = fminf(fmaxf(v, -65504.f), 65504.f);        // fp16 range: saturate, never an (inf, NaN) pair (hosts refuse such weights first)
        const _Float16 hi = (_Float16)v;
        wp[i] = part ? (_Float16)(v - (float)hi) : hi;
        pack_bias(i, bias, ps, Cout, Cout_pad, bp);
    }
}

// Winograd weights (conv3x3_wino.hip): [Cin_pad/16][A][3 ky][part: hi, lo][h = 2][Cout_pad][8 fp16], U = G g along kx in double
struct WinoG { double g[8][3]; int a; };
__global__ void pack_weights_wino_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin, int Cout,
                                         int Cin_pad, int Cout_pad, int ps, WinoG G, _Float16 *__restrict__ wp,
                                         float *__restrict__ bp)
{
    const int A = G.a;
    const int64_t total = (int64_t)Cin_pad * 3 * A * Cout_pad * 2;
    const int Cq_pad = Cout_pad >> 2, Cq = Cout >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int j = t & 7; t >>= 3;
        const int np = (int)(t % Cout_pad); t /= Cout_pad;
        const int h = t & 1; t >>= 1;
        const int part = t & 1; t >>= 1;
        const int ky = (int)(t % 3); t /= 3;
        const int xi = (int)(t % A);
        const int cb = (int)(t / A);
        const int c = cb * 16 + h * 8 + j;
        int n = np;
        bool ok = c < Cin;
        if (ps) {
            const int sub = np / Cq_pad, ch = np - sub * Cq_pad;
            ok = ok && ch < Cq;
            n = 4 * ch + sub;
        } else {
            ok = ok && np < Cout;
        }
        double u = 0.0;
        if (ok) {
            const float *g = w + ((int64_t)n * Cin + c) * 9 + ky * 3;
            u = G.g[xi][0] * (double)g[0] + G.g[xi][1] * (double)g[1] + G.g[xi][2] * (double)g[2];
        }
        // fp16 range: U = G g reaches 1.5x (F(2,3)) .. 15x (F(6,3)) the largest weight.  Saturate instead of packing (inf, NaN); hosts keep
        // such a layer on the direct form (engine.PackedNet tests max |w| x the form's largest |G| row sum against fp16's range)
        u = u > 65504.0 ? 65504.0 : (u < -65504.0 ? -65504.0 : u);
        const _Float16 hi = (_Float16)u;
        wp[i] = part ? (_Float16)(u - (double)hi) : hi;
        pack_bias(i, bias, ps, Cout, Cout_pad, bp);
    }
}

// ---------------------------------------------------------------------------------------------
// clip entry / exit
__global__ void nchw_to_nhwc_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int HW, int Cpad,
                                    int64_t total_pix)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_pix;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / HW, pix = i - f * HW;
        const float *s = src + f * (int64_t)C * HW + pix;
        float *d = dst + i * Cpad;
        for (int c = 0; c < Cpad; ++c) d[c] = c < C ? s[(int64_t)c * HW] : 0.f;
    }
}

__global__ void nhwc_to_nchw_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int HW, int Cpad,
                                    int64_t total_pix, int do_clamp, float lo, float hi)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total_pix;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / HW, pix = i - f * HW;
        const float *s = src + i * Cpad;
        float *d = dst + f * (int64_t)C * HW + pix;
        for (int c = 0; c < C; ++c) {
            float v = s[c];
            if (do_clamp) v = fminf(fmaxf(v, lo), hi);
            d[(int64_t)c * HW] = v;
        }
    }
}

__global__ void halo_pack_kernel(const float *__restrict__ frame, float *__restrict__ dst, int64_t total, int C, int c0,
                                 int n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / n;
        const int c = (int)(i - pix * n);
        dst[i] = frame[pix * C + c0 + c];
    }
}

// split16 half-chunk slice (fold == 8): channels [c0, c0+8) of a split16 frame are two 16-byte pieces of one chunk
// (hi at chunk*16 + half*4 floats, lo 8 floats further); the compact slice stores them as [hi x8 | lo x8] per pixel
__global__ void halo_pack_split8_kernel(const float *__restrict__ frame, float *__restrict__ dst, int64_t HW, int C, int c0,
                                        int unpack)
{
    const int off = (c0 >> 4) * 16 + ((c0 >> 3) & 1) * 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 2 * HW; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i >> 1;
        const int part = (int)(i & 1);                       // 0 = hi, 1 = lo
        float *f = const_cast<float *>(frame) + pix * C + off + part * 8;
        float *d = dst + pix * 8 + part * 4;
        if (unpack) *reinterpret_cast<float4 *>(f) = *reinterpret_cast<const float4 *>(d);
        else *reinterpret_cast<float4 *>(d) = *reinterpret_cast<const float4 *>(f);
    }
}

__global__ void halo_unpack_kernel(const float *__restrict__ src, float *__restrict__ frame, int64_t total, int C, int c0,
                                   int n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / n;
        const int c = (int)(i - pix * n);
        frame[pix * C + c0 + c] = src[i];
    }
}

// uint8 frame I/O: HWC or planar uint8 -> planar fp32 in [0,1] (+ constant trailing channels, e.g. the
// sigma map) and back with the reference's clamp + round-half-even (tensor2img, img_util.py:66,87-90)
__global__ void u8_to_planar_kernel(const uint8_t *__restrict__ src, float *__restrict__ dst, int C, int Cout, int HW,
                                    int hwc, float const_val, int64_t total)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i % HW;
        const int64_t fc = i / HW;
        const int c = (int)(fc % Cout);
        const int64_t f = fc / Cout;
        float v = const_val;
        if (c < C) v = (float)src[hwc ? (f * HW + pix) * C + c : (f * C + c) * HW + pix] / 255.0f;
        dst[i] = v;
    }
}

__global__ void planar_to_u8_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, int C, int HW, int hwc,
                                    int reverse_ch, int64_t total)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i % HW;
        const int64_t fc = i / HW;
        const int c = (int)(fc % C);
        const int64_t f = fc / C;
        const float v = fminf(fmaxf(src[i], 0.f), 1.f) * 255.0f;
        const int co = reverse_ch ? C - 1 - c : c;
        dst[hwc ? (f * HW + pix) * C + co : (f * C + co) * HW + pix] = (uint8_t)rintf(v);
    }
}

// weights of the fused network entry: one thread per (pair, k-step, lane, j): A operand of v_mfma_f32_32x32x16_f16, rows = the
// channel permutation `chan` of conv3x3_kernel (a lane ends with two groups of 8 consecutive channels)
__global__ void pack_head_weights_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin, int Cmid, int Cmid_pad,
                                         _Float16 *__restrict__ wp, float *__restrict__ bp)
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

// Transformed-domain layout (BsvdConvArgs.x_v / y_v, include/bsvd_hip.h): groups per row, floats per frame
static inline int v_groups(int W, int m) { return (((W + m - 1) / m) + 7) / 8 * 8; }
static inline int64_t v_plane_elems(int H, int W, int C, int m) { return (int64_t)H * (v_groups(W, m) / 8) * (C / 16) * v_block_floats(m); }
static inline int64_t v_edge_elems(int H, int W, int C, int m) { return (int64_t)H * ((W + 8 * m - 1) / (8 * m)) * 4 * C; }

// bsvd_to_v: one thread per (frame, row, group, 8-channel block): the A = M + 2 pixels of the group (zero outside the image), BT per channel in
// fp32 (the kernels' WinoForm<M>::input), every transformed value split into an fp16 pair with the kernels' saturating conversions
template <int M>
__global__ void to_v_kernel(const float *__restrict__ x, int64_t x_fs, int x_f32, float *__restrict__ v, int64_t v_fs, int frames, int H, int W,
                            int C, int wg)
{
    constexpr int A = M + 2;
    using F = WinoForm<M>;
    fp16_saturate_on();
    const int c8n = C >> 3;
    const int64_t total = (int64_t)frames * H * wg * c8n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % c8n);
        int64_t r = i / c8n;
        const int g = (int)(r % wg); r /= wg;
        const int row = (int)(r % H);
        const int f = (int)(r / H);
        const int chunk = c8 >> 1, half = c8 & 1;
        float d[A][8];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const int px = M * g - 1 + a;
            const bool ok = px >= 0 && px < W;
            const float *src = x + f * x_fs + ((int64_t)row * W + (ok ? px : 0)) * C;
            if (x_f32) {
#pragma unroll
                for (int k = 0; k < 8; ++k) d[a][k] = ok ? src[c8 * 8 + k] : 0.f;
            } else {
                const _Float16 *hp = reinterpret_cast<const _Float16 *>(src + chunk * 16) + half * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) d[a][k] = ok ? (float)hp[k] + (float)hp[16 + k] : 0.f;
            }
        }
        _Float16 hi[A][8], lo[A][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float din[A], vout[A];
#pragma unroll
            for (int a = 0; a < A; ++a) din[a] = d[a][k];
            F::input(din, vout);
#pragma unroll
            for (int a = 0; a < A; ++a) {
                hi[a][k] = (_Float16)vout[a];
                lo[a][k] = (_Float16)__builtin_fmaf((float)hi[a][k], -1.0f, vout[a]);
            }
        }
        // block (row, tile g / 8, chunk): [position][quarter][8 groups] x 16 B, then the edge line [side][quarter] x 16 B
        constexpr int BLK = v_block_floats(M);
        float *dst = v + f * v_fs + ((int64_t)(row * (wg >> 3) + (g >> 3)) * (C >> 4) + chunk) * BLK;
        const int gl = g & 7;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            *reinterpret_cast<float4 *>(dst + ((a * 4 + half) * 8 + gl) * 4) = *reinterpret_cast<const float4 *>(hi[a]);
            *reinterpret_cast<float4 *>(dst + ((a * 4 + 2 + half) * 8 + gl) * 4) = *reinterpret_cast<const float4 *>(lo[a]);
        }
        if (gl == 0) {
            *reinterpret_cast<float4 *>(dst + A * 128 + half * 4) = *reinterpret_cast<const float4 *>(hi[0]);
            *reinterpret_cast<float4 *>(dst + A * 128 + (2 + half) * 4) = *reinterpret_cast<const float4 *>(lo[0]);
        }
        if (gl == 7) {
            *reinterpret_cast<float4 *>(dst + A * 128 + (4 + half) * 4) = *reinterpret_cast<const float4 *>(hi[A - 1]);
            *reinterpret_cast<float4 *>(dst + A * 128 + (6 + half) * 4) = *reinterpret_cast<const float4 *>(lo[A - 1]);
        }
    }
}

}  // namespace bsvd

using namespace bsvd;

extern "C" {

int bsvd_abi_version(void) { return BSVD_ABI_VERSION; }

int bsvd_conv_args_size(void) { return (int)sizeof(BsvdConvArgs); }

int bsvd_build_info(void)
{
    int v = 0;
#ifdef BSVD_MEASURE
    v |= BSVD_BUILD_MEASURE;
#endif
    return v;
}

const char *bsvd_last_error(void) { return g_err; }

int64_t bsvd_packed_weight_elems(int32_t Cin_pad, int32_t Cout_pad) { return (int64_t)Cin_pad * 9 * Cout_pad; }

// BsvdConvArgs.out_scale / head_out_scale / pre_out_scale: 0 = 1; else a finite, positive, normal, exact power of two
static bool out_scale_ok(float v, float *resolved)
{
    *resolved = v == 0.0f ? 1.0f : v;
    if (v == 0.0f) return true;
    int e;
    return isfinite(v) && v > 0.0f && isnormal(v) && frexpf(v, &e) == 0.5f;
}

static int conv3x3_impl(const BsvdConvArgs *a, void *stream, char *name, int name_len)
{
    if (!a) { set_error("bsvd_conv3x3: args is NULL"); return -1; }
    if (a->dtype != BSVD_F32 && a->dtype != BSVD_F16X3) { set_error("bsvd_conv3x3: dtype %d not supported (BSVD_F32, BSVD_F16X3)", a->dtype); return -2; }
    if (!a->x || !a->y || !(a->w_packed || a->w_wino_packed)) { set_error("bsvd_conv3x3: x, y and w_packed (or w_wino_packed) must be non-NULL"); return -3; }
    if (a->frames <= 0 || a->H <= 0 || a->W <= 0) { set_error("bsvd_conv3x3: bad clip size %d x %d x %d", a->frames, a->H, a->W); return -4; }
    if (a->Cin <= 0 || (a->Cin & 15) || a->Cout <= 0 || (a->Cout & 15)) {
        set_error("bsvd_conv3x3: Cin=%d / Cout=%d must be positive multiples of 16 (pad channels)", a->Cin, a->Cout);
        return -5;
    }
    if (a->stride != 1 && a->stride != 2) { set_error("bsvd_conv3x3: stride %d", a->stride); return -6; }
    if (a->fold < 0 || 2 * a->fold > a->Cin) { set_error("bsvd_conv3x3: fold %d with Cin %d", a->fold, a->Cin); return -7; }
    if (a->act < BSVD_ACT_NONE || a->act > BSVD_ACT_RELU6) { set_error("bsvd_conv3x3: act %d", a->act); return -8; }
    if (a->epilogue < BSVD_EPI_PLAIN || a->epilogue > BSVD_EPI_RESID) { set_error("bsvd_conv3x3: epilogue %d", a->epilogue); return -9; }
    if (a->epilogue == BSVD_EPI_PS_ADD && (a->Cout & 63)) { set_error("bsvd_conv3x3: PS_ADD needs Cout %% 64 == 0, got %d", a->Cout); return -10; }
    if (a->epilogue == BSVD_EPI_RESID && (!a->extra || a->resid_ch < 0 || a->resid_ch > a->Cout)) {
        set_error("bsvd_conv3x3: RESID needs extra and 0 <= resid_ch <= Cout"); return -11;
    }
    if (a->fold > 0) {
        if (a->halo_prev && a->halo_prev_pstride <= 0) { set_error("bsvd_conv3x3: halo_prev_pstride"); return -12; }
        if (a->halo_next && a->halo_next_pstride <= 0) { set_error("bsvd_conv3x3: halo_next_pstride"); return -12; }
    }
    ConvParams p;
    {   // per-layer power-of-two weight scale (ABI v12): checked here, in front of every launch path
        const struct { const char *nm; float v; float *dst; const void *pack; } sc[3] = {
            {"out_scale", a->out_scale, &p.out_scale, a->w_wino_packed ? a->w_wino_packed : a->w_packed},
            {"head_out_scale", a->head_out_scale, &p.head_out_scale, a->head_w_packed},
            {"pre_out_scale", a->pre_out_scale, &p.pre_out_scale, a->pre_w_packed}};
        for (const auto &s : sc) {
            if (!out_scale_ok(s.v, s.dst)) { set_error("bsvd_conv3x3: %s = %g must be 0 (= 1) or a finite, positive, normal power of two", s.nm, (double)s.v); return -23; }
            if (*s.dst == 1.0f) continue;
            if (a->dtype != BSVD_F16X3) { set_error("bsvd_conv3x3: %s = %g: the weight scale is an option of BSVD_F16X3", s.nm, (double)s.v); return -23; }
            if (!s.pack) { set_error("bsvd_conv3x3: %s = %g without the pack it belongs to", s.nm, (double)s.v); return -23; }
        }
        if (p.out_scale != 1.0f && a->w_wino_packed && a->wino_m >= 10 && a->wino_m < 20) {
            set_error("bsvd_conv3x3: out_scale is not available for wino_m %d (the all-positions-per-wave measurement kernel)", a->wino_m); return -23;
        }
        // the unfused planar entry runs head_kernel (conv3x3_edge_f32.hip) on an fp32 pack: it has no scale to undo
        if (p.out_scale != 1.0f && a->x_planar_ch > 0 && !a->head_w_packed) {
            set_error("bsvd_conv3x3: out_scale = %g is not available for the unfused planar entry (x_planar_ch without head_w_packed: an fp32 pack)", (double)p.out_scale); return -23;
        }
    }
    p.x = (const float *)a->x;
    p.halo_prev = a->fold > 0 ? (const float *)a->halo_prev : nullptr;
    p.halo_next = a->fold > 0 ? (const float *)a->halo_next : nullptr;
    p.w = (const float *)(a->w_wino_packed ? a->w_wino_packed : a->w_packed);
    p.wino_m = a->w_wino_packed ? a->wino_m : 0;
    p.fat_min_wgs = a->fat_min_wgs > 0 ? a->fat_min_wgs : 0;
    p.bias = (const float *)a->bias_packed;
    p.extra = (const float *)a->extra;
    p.y = (float *)a->y;
    p.x_fs = a->x_frame_stride; p.extra_fs = a->extra_frame_stride; p.y_fs = a->y_frame_stride;
    p.halo_prev_ps = a->halo_prev_pstride; p.halo_prev_co = a->halo_prev_coff;
    p.halo_next_ps = a->halo_next_pstride; p.halo_next_co = a->halo_next_coff;
    p.extra_ps = a->extra_pstride; p.extra_cs = a->extra_cstride; p.resid_ch = a->resid_ch;
    p.fold = a->fold; p.frames = a->frames; p.H = a->H; p.W = a->W;
    p.Ho = (a->H - 1) / a->stride + 1; p.Wo = (a->W - 1) / a->stride + 1;
    p.Cin = a->Cin; p.Cout = a->Cout; p.act = a->act; p.epilogue = a->epilogue;
    p.ntx = p.nty = p.nct = 0;
    // 16-byte vector gather is legal when every 4-channel group has a single, aligned source
    bool vec = (a->fold & 3) == 0 && (((uintptr_t)a->x) & 15) == 0 && (a->x_frame_stride & 3) == 0;
    if (a->fold > 0 && a->halo_prev)
        vec = vec && (a->halo_prev_pstride & 3) == 0 && (a->halo_prev_coff & 3) == 0 && (((uintptr_t)a->halo_prev) & 15) == 0;
    if (a->fold > 0 && a->halo_next)
        vec = vec && (a->halo_next_pstride & 3) == 0 && (a->halo_next_coff & 3) == 0 && (((uintptr_t)a->halo_next) & 15) == 0;
    p.vec_ok = vec ? 1 : 0;
    p.ablate = 0;
    p.flip = a->tile_order ? 1 : 0;
    p.prec = a->dtype == BSVD_F16X3 ? 1 : 0;
    p.extra_split = a->extra_split;
    p.y_planar_ch = a->y_planar_ch; p.y_clamp = a->y_clamp; p.y_lo = a->y_lo; p.y_hi = a->y_hi;
    p.head_w = nullptr; p.head_bias = nullptr; p.head_cin = 0;
    p.pre_w = nullptr; p.pre_bias = nullptr; p.pre_cin = 0; p.pre_act = 0;
    p.x_f32 = a->x_f32 ? 1 : 0; p.y_f32 = a->y_f32 ? 1 : 0;
    p.x_v = a->x_v; p.y_v = a->y_v; p.v_wg = 0;
    if (a->x_v || a->y_v) {
        const int m = a->wino_m % 10;
        if (a->dtype != BSVD_F16X3 || !a->w_wino_packed) { set_error("bsvd_conv3x3: x_v / y_v are options of the Winograd form (BSVD_F16X3 + w_wino_packed)"); return -22; }
        if ((a->x_v && a->x_v != m) || (a->y_v && a->y_v != m)) { set_error("bsvd_conv3x3: x_v / y_v (%d / %d) must be the form's m = %d", a->x_v, a->y_v, m); return -22; }
        if ((a->x_v && a->x_f32) || (a->y_v && a->y_f32)) { set_error("bsvd_conv3x3: a tensor is either plain fp32 or transformed, not both"); return -22; }
        if (a->y_v && a->epilogue != BSVD_EPI_PLAIN) { set_error("bsvd_conv3x3: y_v needs the PLAIN epilogue"); return -22; }
        if (a->x_v && a->fold > 0 && ((a->halo_prev && ((a->halo_prev_pstride & 15) || (a->halo_prev_coff & 15))) ||
                                      (a->halo_next && ((a->halo_next_pstride & 15) || (a->halo_next_coff & 15))))) {
            set_error("bsvd_conv3x3: x_v halos: pstride and coff are channel counts of transformed tensors (multiples of 16)"); return -22;
        }
        p.v_wg = v_groups(a->W, m);
        const int64_t vfe = v_plane_elems(a->H, a->W, a->x_v ? a->Cin : a->Cout, m);
        if (a->x_v && (a->frames > 1 && a->x_frame_stride < v_plane_elems(a->H, a->W, a->Cin, m))) { set_error("bsvd_conv3x3: x_v: x_frame_stride < the transformed frame"); return -22; }
        if (a->y_v && a->y_frame_stride < bsvd_v_frame_elems(a->H, a->W, a->Cout, m)) { set_error("bsvd_conv3x3: y_v: y_frame_stride < bsvd_v_frame_elems"); return -22; }
        if (vfe * 4 >= 0x7fffffffLL) { set_error("bsvd_conv3x3: transformed frame >= 2 GiB"); return -22; }
    }
    if (a->x_f32 && !(a->dtype == BSVD_F16X3 && a->w_wino_packed)) { set_error("bsvd_conv3x3: x_f32 is the Winograd form's input option (BSVD_F16X3 + w_wino_packed)"); return -21; }
    if (a->y_f32 && (a->dtype != BSVD_F16X3 || a->y_planar_ch > 0 || a->x_planar_ch > 0 || a->epilogue == BSVD_EPI_RESID || a->pre_w_packed || a->head_w_packed ||
                     (a->epilogue == BSVD_EPI_PS_ADD && !a->w_wino_packed))) {
        set_error("bsvd_conv3x3: y_f32 needs BSVD_F16X3 and a PLAIN NHWC layer (direct or Winograd form) or a PS_ADD layer of the Winograd form"); return -21;
    }
    if ((((uintptr_t)p.w) & 15) != 0) { set_error("bsvd_conv3x3: w_packed / w_wino_packed must be 16-byte aligned"); return -13; }
    if (a->w_wino_packed) {      // Winograd form of a wide layer: explicit request, no silent fall-back to the direct kernel
        if (a->x_planar_ch > 0 || a->head_w_packed) { set_error("bsvd_conv3x3: w_wino_packed: not with a planar / fused entry"); return -19; }
        if (const char *why = wino_unsupported(p, a->stride)) { set_error("bsvd_conv3x3: w_wino_packed (F(%d,3)): %s", a->wino_m, why); return -19; }
        // the all-positions-per-wave kernel (conv3x3_wino.hip, measurement builds) knows fp16 pairs only
        if (p.wino_m >= 10 && p.wino_m < 20 && (a->x_f32 || a->y_f32)) { set_error("bsvd_conv3x3: x_f32 / y_f32 are not available for wino_m %d", p.wino_m); return -21; }
        return launch_winox(p, (hipStream_t)stream, name, name_len);
    }
    if (a->pre_w_packed) {       // fused pair of plain stride-1 convs: explicit request, never a silent two-launch fall-back
        if (a->dtype != BSVD_F16X3) { set_error("bsvd_conv3x3: the fused pair (pre_w_packed) is a BSVD_F16X3 kernel"); return -20; }
        if (a->x_planar_ch > 0 || a->head_w_packed) { set_error("bsvd_conv3x3: pre_w_packed: not with a planar input / fused entry"); return -20; }
        if (a->stride != 1 || a->fold != 0 || a->epilogue == BSVD_EPI_PS_ADD) { set_error("bsvd_conv3x3: fused pair needs stride 1, fold 0, PLAIN / RESID"); return -20; }
        // (Cin <= 64: the kernel carries TWO 32-channel pairs of the first conv's output -- pair 0 in the patch buffers, pair 1 in registers;
        //  a wider middle tensor would refill chunks 4.. with pair 1's data: refused, never silently wrong)
        if (a->pre_cin <= 0 || (a->pre_cin & 15) || (a->Cin & 31) || a->Cin > 64 || a->Cout > 64) {
            set_error("bsvd_conv3x3: fused pair needs pre_cin %% 16 == 0, Cin = 32 or 64, Cout <= 64 (pre_cin %d, Cin %d, Cout %d)", a->pre_cin, a->Cin, a->Cout); return -20;
        }
        if (a->pre_act < BSVD_ACT_NONE || a->pre_act > BSVD_ACT_RELU6) { set_error("bsvd_conv3x3: pre_act %d", a->pre_act); return -20; }
        if (!a->pre_bias || (((uintptr_t)a->pre_w_packed) & 15) || (((uintptr_t)a->pre_bias) & 15) || (((uintptr_t)a->x) & 15) || (a->x_frame_stride & 3)) {
            set_error("bsvd_conv3x3: fused pair needs 16-byte aligned x, pre_w_packed and pre_bias"); return -20;
        }
        if ((int64_t)a->H * a->W * (a->pre_cin > a->Cout ? a->pre_cin : a->Cout) * 4 >= 0x7fffffffLL ||
            (int64_t)a->pre_cin * 9 * a->Cin * 4 >= 0x7fffffffLL) { set_error("bsvd_conv3x3: frame / weights too large for the fused pair (2 GiB byte offsets)"); return -20; }
        p.pre_w = a->pre_w_packed; p.pre_bias = (const float *)a->pre_bias; p.pre_cin = a->pre_cin; p.pre_act = a->pre_act;
        p.vec_ok = 1;
        if (a->y_planar_ch > 0) {
            if (a->Cout != 16 || a->y_planar_ch > 4 || (a->epilogue == BSVD_EPI_RESID && a->resid_ch > a->y_planar_ch)) { set_error("bsvd_conv3x3: fused pair with a planar output needs Cout == 16 and 1..4 planar channels"); return -20; }
        }
        return launch_conv3x3(p, 1, (hipStream_t)stream, name, name_len);
    }
    if (a->x_planar_ch > 0 || a->y_planar_ch > 0) {
        if (a->x_planar_ch > 0 && a->y_planar_ch > 0) { set_error("bsvd_conv3x3: x_planar_ch and y_planar_ch are exclusive"); return -16; }
        if (a->stride != 1 || a->fold != 0) { set_error("bsvd_conv3x3: planar edge layers need stride 1 and fold 0"); return -16; }
        if ((int64_t)a->H * a->W * (a->Cin > a->Cout ? a->Cin : a->Cout) >= 0x7fffffffLL) { set_error("bsvd_conv3x3: frame too large for the edge kernels"); return -16; }
        if (a->x_planar_ch > 0 && a->head_w_packed) {
            // fused network entry: planar input -> (x_planar_ch -> Cin conv, act) -> (Cin -> Cout conv, act), one launch
            if (a->dtype != BSVD_F16X3) { set_error("bsvd_conv3x3: the fused entry (head_w_packed) is a BSVD_F16X3 kernel"); return -18; }
            if (a->x_planar_ch != 3 && a->x_planar_ch != 4) { set_error("bsvd_conv3x3: fused entry supports 3 or 4 planar input channels, got %d", a->x_planar_ch); return -18; }
            if ((a->Cin & 31) || a->Cout > 64 || a->epilogue != BSVD_EPI_PLAIN || a->y_planar_ch > 0) {
                set_error("bsvd_conv3x3: fused entry needs Cin %% 32 == 0, Cout <= 64 and the PLAIN epilogue (Cin %d, Cout %d)", a->Cin, a->Cout); return -18;
            }
            if (!a->head_bias || (((uintptr_t)a->head_w_packed) & 15) || (((uintptr_t)a->head_bias) & 15)) { set_error("bsvd_conv3x3: fused entry needs 16-byte aligned head_w_packed and head_bias"); return -18; }
            if ((int64_t)a->H * a->W * a->Cout * 4 >= 0x7fffffffLL) { set_error("bsvd_conv3x3: frame too large for the fused entry"); return -18; }
            p.head_w = a->head_w_packed; p.head_bias = (const float *)a->head_bias; p.head_cin = a->x_planar_ch;
            p.vec_ok = 1;
            return launch_conv3x3(p, 1, (hipStream_t)stream, name, name_len);
        }
        if (a->x_planar_ch > 0) {
            if (a->Cin != 16 || a->epilogue != BSVD_EPI_PLAIN) { set_error("bsvd_conv3x3: planar input needs Cin == 16 (padded) and the PLAIN epilogue"); return -16; }
            if (name) { snprintf(name, name_len, "head_kernel<%d>%s", a->x_planar_ch, p.prec == 1 ? "[f16x3 out]" : "[f32]"); return 0; }
            return launch_head_f32(p, a->x_planar_ch, (hipStream_t)stream);
        }
        if (a->Cout != 16 || a->epilogue == BSVD_EPI_PS_ADD) { set_error("bsvd_conv3x3: planar output needs Cout == 16 (padded) and PLAIN/RESID"); return -16; }
        if (a->epilogue == BSVD_EPI_RESID && a->resid_ch > a->y_planar_ch) { set_error("bsvd_conv3x3: resid_ch > y_planar_ch"); return -16; }
        if (a->y_planar_ch > 4) { set_error("bsvd_conv3x3: planar output supports 1..4 channels, got %d", a->y_planar_ch); return -15; }
        // split16: the exit layer runs on the matrix cores too (one 32-channel column tile, 3-4 of them live; weights
        // split-packed like every other BSVD_F16X3 layer) and writes planar fp32 from its epilogue
        if (p.prec == 1) return launch_conv3x3(p, 1, (hipStream_t)stream, name, name_len);
        if (name) { snprintf(name, name_len, "tail_kernel<%d>[f32]", a->y_planar_ch == 3 ? 3 : 4); return 0; }
        return launch_tail_f32(p, a->y_planar_ch, a->y_clamp, a->y_lo, a->y_hi, (hipStream_t)stream);
    }
    return launch_conv3x3(p, a->stride, (hipStream_t)stream, name, name_len);
}

int bsvd_conv3x3(const BsvdConvArgs *a, void *stream) { return conv3x3_impl(a, stream, nullptr, 0); }

int32_t bsvd_v_groups(int32_t W, int32_t m) { return (m == 2 || m == 4 || m == 6) && W > 0 ? v_groups(W, m) : -1; }

int64_t bsvd_v_frame_elems(int32_t H, int32_t W, int32_t C, int32_t m)
{
    if (!(m == 2 || m == 4 || m == 6) || H <= 0 || W <= 0 || C <= 0 || (C & 15)) { set_error("bsvd_v_frame_elems: m = 2 | 4 | 6, C %% 16 == 0"); return -1; }
    return v_plane_elems(H, W, C, m) + v_edge_elems(H, W, C, m);
}

int bsvd_to_v(const void *x, int64_t x_fs, int32_t x_f32, void *v, int64_t v_fs, int32_t frames, int32_t H, int32_t W, int32_t C, int32_t m,
              void *stream)
{
    if (!x || !v || frames <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 15)) { set_error("bsvd_to_v: bad arguments (C %% 16 == 0)"); return -3; }
    if (!(m == 2 || m == 4 || m == 6)) { set_error("bsvd_to_v: m = %d (2, 4 or 6)", m); return -2; }
    if ((((uintptr_t)x) & 15) || (((uintptr_t)v) & 15) || (v_fs & 3)) { set_error("bsvd_to_v: 16-byte aligned tensors"); return -3; }
    if (v_fs < bsvd_v_frame_elems(H, W, C, m)) { set_error("bsvd_to_v: v_frame_stride < bsvd_v_frame_elems"); return -3; }
    const int wg = v_groups(W, m);
    hipError_t e = hipMemsetAsync(v, 0, (size_t)frames * v_fs * 4, (hipStream_t)stream);        // pad groups and the edge record: zeros
    if (e != hipSuccess) return (int)e;
    const int64_t total = (int64_t)frames * H * wg * (C >> 3);
    if (m == 2) hipLaunchKernelGGL(to_v_kernel<2>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float *)x, x_fs, x_f32, (float *)v, v_fs, frames, H, W, C, wg);
    else if (m == 4) hipLaunchKernelGGL(to_v_kernel<4>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float *)x, x_fs, x_f32, (float *)v, v_fs, frames, H, W, C, wg);
    else hipLaunchKernelGGL(to_v_kernel<6>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float *)x, x_fs, x_f32, (float *)v, v_fs, frames, H, W, C, wg);
    return (int)hipGetLastError();
}

int bsvd_conv3x3_variant(const BsvdConvArgs *a, char *name, int32_t name_len)
{
    if (!name || name_len < 8) { set_error("bsvd_conv3x3_variant: name buffer too small"); return -1; }
    name[0] = 0;
    return conv3x3_impl(a, nullptr, name, name_len);
}

int64_t bsvd_packed_wino_weight_elems(int32_t Cin_pad, int32_t Cout_pad, int32_t m) { return (int64_t)Cin_pad * 3 * (m + 2) * Cout_pad; }

int bsvd_pack_weights_wino(const float *w, const float *bias, int32_t Cin, int32_t Cout, int32_t Cin_pad, int32_t Cout_pad,
                           int32_t pixel_shuffle, int32_t m, void *wp, void *bp, void *stream)
{
    if (m != 2 && m != 4 && m != 6) { set_error("bsvd_pack_weights_wino: m = %d (2, 4 or 6)", m); return -2; }
    if (!w || !wp) { set_error("bsvd_pack_weights_wino: NULL weight pointer"); return -3; }
    if (Cin <= 0 || Cout <= 0 || Cin_pad < Cin || Cout_pad < Cout || (Cin_pad & 15) || (Cout_pad & 31)) {
        set_error("bsvd_pack_weights_wino: bad sizes Cin %d->%d Cout %d->%d (Cin_pad %% 16, Cout_pad %% 32)", Cin, Cin_pad, Cout, Cout_pad); return -5;
    }
    if (pixel_shuffle && ((Cout & 3) || (Cout_pad & 63))) { set_error("bsvd_pack_weights_wino: pixel_shuffle needs Cout %% 4 == 0 and Cout_pad %% 64 == 0"); return -10; }
    WinoG G;
    G.a = m + 2;
    for (int x = 0; x < 8; ++x)
        for (int k = 0; k < 3; ++k)
            G.g[x][k] = x >= m + 2 ? 0.0 : (m == 6 ? WinoForm<6>::G[x][k] : m == 4 ? WinoForm<4>::G[x < 6 ? x : 0][k] : WinoForm<2>::G[x < 4 ? x : 0][k]);
    const int64_t total = (int64_t)Cin_pad * 3 * (m + 2) * Cout_pad * 2;
    hipLaunchKernelGGL(pack_weights_wino_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, w, bias, Cin, Cout,
                       Cin_pad, Cout_pad, pixel_shuffle ? 1 : 0, G, (_Float16 *)wp, (float *)bp);
    return (int)hipGetLastError();
}

int bsvd_pack_weights(const float *w, const float *bias, int32_t Cin, int32_t Cout, int32_t Cin_pad, int32_t Cout_pad,
                      int32_t pixel_shuffle, int32_t dtype, void *wp, void *bp, void *stream)
{
    if (dtype != BSVD_F32 && dtype != BSVD_F16X3) { set_error("bsvd_pack_weights: dtype %d not supported", dtype); return -2; }
    if (!w || !wp) { set_error("bsvd_pack_weights: NULL weight pointer"); return -3; }
    if (Cin <= 0 || Cout <= 0 || Cin_pad < Cin || Cout_pad < Cout || (Cin_pad & 15) || (Cout_pad & 15)) {
        set_error("bsvd_pack_weights: bad sizes Cin %d->%d Cout %d->%d", Cin, Cin_pad, Cout, Cout_pad); return -5;
    }
    if (pixel_shuffle && ((Cout & 3) || (Cout_pad & 63) || (Cout_pad >> 2) < (Cout >> 2))) {
        set_error("bsvd_pack_weights: pixel_shuffle needs Cout %% 4 == 0 and Cout_pad %% 64 == 0"); return -10;
    }
    const int64_t total = bsvd_packed_weight_elems(Cin_pad, Cout_pad);
    if (dtype == BSVD_F16X3) {
        hipLaunchKernelGGL(pack_weights_split_kernel, dim3(grid_for(2 * total, 256)), dim3(256), 0, (hipStream_t)stream, w,
                           bias, Cin, Cout, Cin_pad, Cout_pad, pixel_shuffle ? 1 : 0, (_Float16 *)wp, (float *)bp);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(pack_weights_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, w, bias, Cin,
                       Cout, Cin_pad, Cout_pad, pixel_shuffle ? 1 : 0, (float *)wp, (float *)bp);
    return (int)hipGetLastError();
}

int64_t bsvd_packed_head_weight_bytes(int32_t Cmid_pad) { return (int64_t)(Cmid_pad / 32) * 3 * 64 * 32; }

int bsvd_pack_head_weights(const float *w, const float *bias, int32_t Cin, int32_t Cmid, int32_t Cmid_pad, void *wp, float *bp,
                           void *stream)
{
    if (!w || !wp || !bp) { set_error("bsvd_pack_head_weights: NULL pointer"); return -3; }
    if ((Cin != 3 && Cin != 4) || Cmid <= 0 || Cmid_pad < Cmid || (Cmid_pad & 31)) {
        set_error("bsvd_pack_head_weights: needs Cin 3|4 and Cmid_pad %% 32 == 0 (Cin %d, Cmid %d -> %d)", Cin, Cmid, Cmid_pad); return -5;
    }
    hipLaunchKernelGGL(pack_head_weights_kernel, dim3(grid_for((int64_t)(Cmid_pad / 32) * 3 * 64 * 8, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, bias, Cin, Cmid, Cmid_pad, (_Float16 *)wp, bp);
    return (int)hipGetLastError();
}

int bsvd_nchw_to_nhwc(const float *src, void *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t C_pad,
                      int32_t dtype, void *stream)
{
    if (dtype != BSVD_F32) { set_error("bsvd_nchw_to_nhwc: dtype %d not supported", dtype); return -2; }
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || C_pad < C) { set_error("bsvd_nchw_to_nhwc: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * H * W;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       (float *)dst, C, H * W, C_pad, total);
    return (int)hipGetLastError();
}

int bsvd_nhwc_to_nchw(const void *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t C_pad,
                      int32_t dtype, int32_t do_clamp, float lo, float hi, void *stream)
{
    if (dtype != BSVD_F32) { set_error("bsvd_nhwc_to_nchw: dtype %d not supported", dtype); return -2; }
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || C_pad < C) { set_error("bsvd_nhwc_to_nchw: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * H * W;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)src, dst, C, H * W, C_pad, total, do_clamp, lo, hi);
    return (int)hipGetLastError();
}

int bsvd_u8_to_planar(const uint8_t *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t src_hwc,
                      int32_t const_channels, float const_val, void *stream)
{
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0 || const_channels < 0) { set_error("bsvd_u8_to_planar: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * (C + const_channels) * H * W;
    hipLaunchKernelGGL(u8_to_planar_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, C,
                       C + const_channels, H * W, src_hwc ? 1 : 0, const_val, total);
    return (int)hipGetLastError();
}

int bsvd_planar_to_u8(const float *src, uint8_t *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t dst_hwc,
                      int32_t reverse_channels, void *stream)
{
    if (!src || !dst || frames <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("bsvd_planar_to_u8: bad arguments"); return -3; }
    const int64_t total = (int64_t)frames * C * H * W;
    hipLaunchKernelGGL(planar_to_u8_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, C, H * W,
                       dst_hwc ? 1 : 0, reverse_channels ? 1 : 0, total);
    return (int)hipGetLastError();
}

int bsvd_halo_pack(const void *frame, void *dst, int32_t HW, int32_t C, int32_t c0, int32_t n, int32_t dtype,
                   void *stream)
{
    if (dtype != BSVD_F32 && dtype != BSVD_F16X3) { set_error("bsvd_halo_pack: dtype %d not supported", dtype); return -2; }
    if (!frame || !dst || HW <= 0 || C <= 0 || c0 < 0 || n <= 0 || c0 + n > C) { set_error("bsvd_halo_pack: bad arguments"); return -3; }
    if (dtype == BSVD_F16X3) {         // half-chunk slice of a split16 frame (whole chunks are plain float ranges: use BSVD_F32)
        if (n != 8 || (c0 & 7) || (C & 15)) { set_error("bsvd_halo_pack: BSVD_F16X3 packs one 8-channel half chunk (n == 8, c0 %% 8 == 0)"); return -3; }
        hipLaunchKernelGGL(halo_pack_split8_kernel, dim3(grid_for(2 * (int64_t)HW, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float *)frame, (float *)dst, (int64_t)HW, C, c0, 0);
        return (int)hipGetLastError();
    }
    const int64_t total = (int64_t)HW * n;
    hipLaunchKernelGGL(halo_pack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)frame, (float *)dst, total, C, c0, n);
    return (int)hipGetLastError();
}

int bsvd_halo_unpack(const void *src, void *frame, int32_t HW, int32_t C, int32_t c0, int32_t n, int32_t dtype,
                     void *stream)
{
    if (dtype != BSVD_F32 && dtype != BSVD_F16X3) { set_error("bsvd_halo_unpack: dtype %d not supported", dtype); return -2; }
    if (!frame || !src || HW <= 0 || C <= 0 || c0 < 0 || n <= 0 || c0 + n > C) { set_error("bsvd_halo_unpack: bad arguments"); return -3; }
    if (dtype == BSVD_F16X3) {
        if (n != 8 || (c0 & 7) || (C & 15)) { set_error("bsvd_halo_unpack: BSVD_F16X3 unpacks one 8-channel half chunk (n == 8, c0 %% 8 == 0)"); return -3; }
        hipLaunchKernelGGL(halo_pack_split8_kernel, dim3(grid_for(2 * (int64_t)HW, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float *)frame, const_cast<float *>((const float *)src), (int64_t)HW, C, c0, 1);
        return (int)hipGetLastError();
    }
    const int64_t total = (int64_t)HW * n;
    hipLaunchKernelGGL(halo_unpack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)src, (float *)frame, total, C, c0, n);
    return (int)hipGetLastError();
}

int64_t bsvd_workspace_bytes(const BsvdConvArgs *args)
{
    char name[8];
    const int rc = bsvd_conv3x3_variant(args, name, (int32_t)sizeof(name));   // argument validation only, no launch
    return rc < 0 ? (int64_t)rc : 0;
}

// ---------------------------------------------------------------------------------------------
// one streaming step as one submission: batch launch + HIP graph capture / replay
int bsvd_conv3x3_batch(const BsvdConvArgs *args, int32_t n, void *stream)
{
    if (n < 0 || (n > 0 && !args)) { set_error("bsvd_conv3x3_batch: bad arguments"); return -1; }
    for (int32_t i = 0; i < n; ++i) {
        const int rc = conv3x3_impl(args + i, stream, nullptr, 0);
        if (rc != 0) {
            if (rc < 0) {
                char msg[400];
                snprintf(msg, sizeof(msg), "%s", g_err);
                set_error("bsvd_conv3x3_batch: layer %d of %d: %s", i, n, msg);
            }
            return rc;
        }
    }
    return 0;
}

int bsvd_graph_begin(void *capture_stream)
{
    if (!capture_stream) { set_error("bsvd_graph_begin: the default stream cannot be captured; pass a created stream"); return -1; }
    return (int)hipStreamBeginCapture((hipStream_t)capture_stream, hipStreamCaptureModeRelaxed);
}

static int graph_edge(hipStream_t from, hipStream_t to)
{
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return (int)e;
    e = hipEventRecord(ev, from);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
    (void)hipEventDestroy(ev);      // the dependency edge lives in the capturing graph, not in the event
    return (int)e;
}

int bsvd_graph_fork(void *capture_stream, void *side_stream)
{
    if (!capture_stream || !side_stream) { set_error("bsvd_graph_fork: NULL stream"); return -1; }
    return graph_edge((hipStream_t)capture_stream, (hipStream_t)side_stream);
}

int bsvd_graph_join(void *capture_stream, void *side_stream)
{
    if (!capture_stream || !side_stream) { set_error("bsvd_graph_join: NULL stream"); return -1; }
    return graph_edge((hipStream_t)side_stream, (hipStream_t)capture_stream);
}

int bsvd_graph_end(void *capture_stream, void **graph_exec, int32_t *num_nodes)
{
    if (!capture_stream || !graph_exec) { set_error("bsvd_graph_end: NULL argument"); return -1; }
    *graph_exec = nullptr;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture((hipStream_t)capture_stream, &g);
    if (e != hipSuccess || !g) return e != hipSuccess ? (int)e : (int)hipErrorUnknown;
    if (num_nodes) {
        size_t n = 0;
        (void)hipGraphGetNodes(g, nullptr, &n);
        *num_nodes = (int32_t)n;
    }
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return (int)e;
    *graph_exec = ex;
    return 0;
}

int bsvd_graph_abort(void *capture_stream)
{
    if (!capture_stream) return -1;
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture((hipStream_t)capture_stream, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    return 0;
}

int bsvd_graph_launch(void *graph_exec, void *stream)
{
    if (!graph_exec) { set_error("bsvd_graph_launch: NULL graph"); return -1; }
    return (int)hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
}

int bsvd_graph_destroy(void *graph_exec)
{
    if (!graph_exec) return 0;
    return (int)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
}

}  // extern "C"
