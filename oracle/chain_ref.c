/* CPU MODEL OF THE EXACT-fp32 MODE (plain C) -- TEST INFRASTRUCTURE ONLY, never linked into the product library.
 *
 * The same layer as oracle_conv3x3 (oracle/conv_ref.c: gather with fold and two nullable halo slices, stride 1 | 2, bias,
 * activation, epilogues 0 / 1 / 2), but in the arithmetic include/bsvd_hip.h documents for dtype BSVD_F32 ("Arithmetic of
 * BSVD_F32"): every operation is ONE single-precision fmaf() or ONE fp32 add / subtract, in a stated order, so that a kernel
 * of that mode can be compared with it bit for bit.  No doubles anywhere; explicit fmaf calls, so the result does not depend
 * on -ffp-contract.
 *
 *   accumulator : starts at +0 (flag CHAIN_BIAS_FIRST: at the bias)
 *   terms       : the input is the gathered frame, zero-padded to Cp = 16 * ceil(Cin / 16) channels.  EVERY (chunk, tap, channel)
 *                 of it is a term acc = fmaf(x, w, acc); taps outside the image and padded channels are terms with a zero operand.
 *   order       : CHAIN_ORDER_MFMA  for chunk c, tap t = 3 ky + kx, g in 0..1, j in 0..3:
 *                                       channel 16c + 8g + j, then channel 16c + 8g + 4 + j
 *                                   (the two k of one v_mfma_f32_32x32x2_f32; CHAIN_SWAP_K: the second one first)
 *                 CHAIN_ORDER_EDGE  for chunk c, tap t, channel 16c + 0 .. 16c + 15
 *   epilogue    : v = acc + bias (one rounding; skipped under CHAIN_BIAS_FIRST), activation (max(v, 0), then min(v, 6)),
 *                 PS_ADD v + skip, RESID extra - v on the first resid_ch channels, optional clamp min(max(v, lo), hi).
 *
 * The remaining flags are MUTATIONS: wrong kernels for tests/test_fp32_chain_cpu.py to show that the assertions of
 * tests/test_gpu_fp32_chain.py would catch them.
 *
 * Layout: NCHW, one frame per call, as oracle_conv3x3.
 * Build: gcc -O2 -fopenmp -shared -fPIC oracle/chain_ref.c -o oracle/libchain_ref.so -lm
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { CHAIN_ORDER_MFMA = 0, CHAIN_ORDER_EDGE = 1 };
enum {
    CHAIN_SWAP_K = 1,       /* documented-open: the two k of one MFMA in the other order                     */
    CHAIN_BIAS_FIRST = 2,   /* documented-open: the accumulator starts at the bias, no add behind the chain   */
    CHAIN_TAP_MAJOR = 4,    /* mutation: (tap, chunk, ...) instead of (chunk, tap, ...)                       */
    CHAIN_ROUND11 = 8,      /* mutation: both operands rounded to an 11-bit significand (fp16's)              */
    CHAIN_DROP_TERM = 16    /* mutation: the term (channel 1, centre tap) is missing                          */
};

static inline float round11(float v)
{
    /* round to nearest even at 11 significant bits, exponent range untouched (finite inputs) */
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint32_t drop = 13, half = 1u << (drop - 1), lsb = (u >> drop) & 1u;
    u += half - 1u + lsb;
    u &= ~((1u << drop) - 1u);
    memcpy(&v, &u, 4);
    return v;
}

/* returns 0 on success, -1 on bad arguments, -2 out of memory */
int chain_conv3x3(const float *cur,      /* [Cin][H][W]                                                     */
                  const float *prev_sl,  /* [fold][H][W] = prev frame ch fold..2fold-1, or NULL             */
                  const float *next_sl,  /* [fold][H][W] = next frame ch 0..fold-1,     or NULL             */
                  int fold, const float *w /* [Cout][Cin][3][3] */, const float *bias /* [Cout] or NULL */,
                  int Cin, int Cout, int H, int W, int stride, int act, int epilogue,
                  const float *extra,    /* epilogue 1: skip [Cout/4][2Ho][2Wo] or NULL; 2: base [>= resid_ch][Ho][Wo] */
                  float *out,            /* epi 0/2: [Cout][Ho][Wo]; epi 1: [Cout/4][2Ho][2Wo]             */
                  int resid_ch, int do_clamp, float lo, float hi, int order, int flags)
{
    if (!cur || !w || !out || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return -1;
    if (fold < 0 || 2 * fold > Cin || H <= 0 || W <= 0) return -1;
    if (epilogue == 1 && (Cout % 4)) return -1;
    if (epilogue == 2 && (!extra || resid_ch < 0)) return -1;
    if (order != CHAIN_ORDER_MFMA && order != CHAIN_ORDER_EDGE) return -1;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int Cp = (Cin + 15) / 16 * 16, nchunk = Cp / 16;
    const int Hp = H + 2, Wp = W + 2;
    const size_t plane = (size_t)H * W, pplane = (size_t)Hp * Wp;

    /* the gathered frame with its zero border and zero padding channels: [Cp][H + 2][W + 2] */
    float *g = (float *)calloc((size_t)Cp * pplane, sizeof(float));
    float *wz = (float *)calloc((size_t)Cout * Cp * 9, sizeof(float));      /* [Cout][Cp][9] */
    if (!g || !wz) { free(g); free(wz); return -2; }
    for (int ci = 0; ci < Cin; ++ci) {
        const float *src;
        if (ci < fold)            src = next_sl ? next_sl + (size_t)ci * plane : NULL;
        else if (ci < 2 * fold)   src = prev_sl ? prev_sl + (size_t)(ci - fold) * plane : NULL;
        else                      src = cur + (size_t)ci * plane;
        if (!src) continue;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                float v = src[(size_t)y * W + x];
                if (flags & CHAIN_ROUND11) v = round11(v);
                g[(size_t)ci * pplane + (size_t)(y + 1) * Wp + (x + 1)] = v;
            }
    }
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < 9; ++t) {
                float v = w[((size_t)co * Cin + ci) * 9 + t];
                if (flags & CHAIN_ROUND11) v = round11(v);
                if ((flags & CHAIN_DROP_TERM) && ci == (Cin > 1 ? 1 : 0) && t == 4) v = 0.0f;
                wz[((size_t)co * Cp + ci) * 9 + t] = v;
            }

    /* channel order inside one 16-channel chunk */
    int perm[16];
    for (int g2 = 0; g2 < 2; ++g2)
        for (int j = 0; j < 4; ++j) {
            const int k0 = 8 * g2 + j, k1 = 8 * g2 + 4 + j, i = 2 * (4 * g2 + j);
            perm[i] = (flags & CHAIN_SWAP_K) ? k1 : k0;
            perm[i + 1] = (flags & CHAIN_SWAP_K) ? k0 : k1;
        }
    if (order == CHAIN_ORDER_EDGE)
        for (int i = 0; i < 16; ++i) perm[i] = i;

#pragma omp parallel for schedule(static)
    for (int co = 0; co < Cout; ++co) {
        const float *wc = wz + (size_t)co * Cp * 9;
        for (int oy = 0; oy < Ho; ++oy) {
            for (int ox = 0; ox < Wo; ++ox) {
                const float *gp = g + (size_t)(oy * stride) * Wp + (size_t)(ox * stride);   /* tap (0, 0) of this output */
                float acc = ((flags & CHAIN_BIAS_FIRST) && bias) ? bias[co] : 0.0f;
                if (!(flags & CHAIN_TAP_MAJOR)) {
                    for (int c = 0; c < nchunk; ++c)
                        for (int t = 0; t < 9; ++t) {
                            const size_t toff = (size_t)(t / 3) * Wp + (size_t)(t % 3);
                            for (int i = 0; i < 16; ++i) {
                                const int ci = 16 * c + perm[i];
                                acc = fmaf(gp[(size_t)ci * pplane + toff], wc[(size_t)ci * 9 + t], acc);
                            }
                        }
                } else {
                    for (int t = 0; t < 9; ++t) {
                        const size_t toff = (size_t)(t / 3) * Wp + (size_t)(t % 3);
                        for (int c = 0; c < nchunk; ++c)
                            for (int i = 0; i < 16; ++i) {
                                const int ci = 16 * c + perm[i];
                                acc = fmaf(gp[(size_t)ci * pplane + toff], wc[(size_t)ci * 9 + t], acc);
                            }
                    }
                }
                float v = acc;
                if (!(flags & CHAIN_BIAS_FIRST) && bias) v = acc + bias[co];
                if (act >= 1) v = fmaxf(v, 0.0f);
                if (act == 2) v = fminf(v, 6.0f);
                size_t o;
                if (epilogue == 1) {
                    const int c = co >> 2, i = (co >> 1) & 1, j = co & 1;
                    o = ((size_t)c * (2 * Ho) + (2 * oy + i)) * (2 * Wo) + (2 * ox + j);
                    if (extra) v = v + extra[o];
                } else {
                    o = ((size_t)co * Ho + oy) * Wo + ox;
                    if (epilogue == 2 && co < resid_ch) v = extra[o] - v;
                }
                if (do_clamp) v = fminf(fmaxf(v, lo), hi);
                out[o] = v;
            }
        }
    }
    free(g);
    free(wz);
    return 0;
}
