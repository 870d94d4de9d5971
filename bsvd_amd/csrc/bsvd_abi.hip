// bsvd_abi.hip -- the conv entry of libbsvd_hip.so (see include/bsvd_hip.h): error text, version and build info, the checks of
// BsvdConvArgs, dispatch to the four launchers, the batch call and HIP graph capture / replay.  The weight packs live in weight_pack.hip,
// the layout helpers in tensor_layout.hip, YUV frame I/O in frame_yuv.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include "bsvd_internal.h"

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
// conv3x3_check: BsvdConvArgs -> ConvParams + Route, or a negative code with the reason in g_err.  No launch, no allocation, no formatting
// on the success path.  The check functions run in the order below and the first refusal wins; each returns 0 to go on.
enum RouteKind { ROUTE_CONV, ROUTE_WINO, ROUTE_HEAD_F32, ROUTE_TAIL_F32 };
// kind: launch_conv3x3 (direct form: MFMA or exact fp32) | launch_winox | launch_head_f32 | launch_tail_f32; arg: that launcher's extra
// argument -- the stride (ROUTE_CONV) or the planar channel count (the fp32 edge kernels)
struct Route { RouteKind kind; int arg; };

static int check_common(const BsvdConvArgs *a)
{
    if (!a) { set_error("bsvd_conv3x3: args is NULL"); return -1; }
    if (a->dtype != BSVD_F32 && a->dtype != BSVD_F16X3 && a->dtype != BSVD_F16) { set_error("bsvd_conv3x3: dtype %d not supported (BSVD_F32, BSVD_F16X3)", a->dtype); return -2; }
    if (!a->x || !a->y || !(a->w_packed || a->w_wino_packed)) { set_error("bsvd_conv3x3: x, y and w_packed (or w_wino_packed) must be non-NULL"); return -3; }
    if (a->frames <= 0 || a->H <= 0 || a->W <= 0) { set_error("bsvd_conv3x3: bad clip size %d x %d x %d", a->frames, a->H, a->W); return -4; }
    if (a->Cin <= 0 || (a->Cin & 15) || a->Cout <= 0 || (a->Cout & 15)) { set_error("bsvd_conv3x3: Cin=%d / Cout=%d must be positive multiples of 16 (pad channels)", a->Cin, a->Cout); return -5; }
    if (a->stride != 1 && a->stride != 2) { set_error("bsvd_conv3x3: stride %d", a->stride); return -6; }
    if (a->fold < 0 || 2 * a->fold > a->Cin) { set_error("bsvd_conv3x3: fold %d with Cin %d", a->fold, a->Cin); return -7; }
    if (a->act < BSVD_ACT_NONE || a->act > BSVD_ACT_RELU6) { set_error("bsvd_conv3x3: act %d", a->act); return -8; }
    if (a->epilogue < BSVD_EPI_PLAIN || a->epilogue > BSVD_EPI_RESID) { set_error("bsvd_conv3x3: epilogue %d", a->epilogue); return -9; }
    if (a->epilogue == BSVD_EPI_PS_ADD && (a->Cout & 63)) { set_error("bsvd_conv3x3: PS_ADD needs Cout %% 64 == 0, got %d", a->Cout); return -10; }
    if (a->epilogue == BSVD_EPI_RESID && (!a->extra || a->resid_ch < 0 || a->resid_ch > a->Cout)) { set_error("bsvd_conv3x3: RESID needs extra and 0 <= resid_ch <= Cout"); return -11; }
    if (a->fold > 0 && a->halo_prev && a->halo_prev_pstride <= 0) { set_error("bsvd_conv3x3: halo_prev_pstride"); return -12; }
    if (a->fold > 0 && a->halo_next && a->halo_next_pstride <= 0) { set_error("bsvd_conv3x3: halo_next_pstride"); return -12; }
    return 0;
}

// BsvdConvArgs.out_scale / head_out_scale / pre_out_scale: 0 = 1; else a finite, positive, normal, exact power of two
static bool out_scale_ok(float v, float *resolved)
{
    int e;
    *resolved = v == 0.0f ? 1.0f : v;
    return v == 0.0f || (isfinite(v) && v > 0.0f && isnormal(v) && frexpf(v, &e) == 0.5f);
}

// the split modes share one data contract: BSVD_F16X3 (three MFMA passes) and BSVD_F16 (one pass on the same containers and packs)
static inline bool split_dtype(int dtype) { return dtype == BSVD_F16X3 || dtype == BSVD_F16; }

// BSVD_F16: what the one-pass mode does not instantiate is refused here, before any launch, with a code of its own and the option's name
static int check_one_pass(const BsvdConvArgs *a)
{
    if (a->dtype != BSVD_F16) return 0;
    if (a->pre_w_packed) { set_error("bsvd_conv3x3: BSVD_F16: the fused pair (pre_w_packed) is a BSVD_F16X3 kernel only"); return -24; }
    if (a->x_v || a->y_v) { set_error("bsvd_conv3x3: BSVD_F16: transformed-domain tensors (x_v / y_v = %d / %d) are BSVD_F16X3 options only", a->x_v, a->y_v); return -24; }
    if (a->w_wino_packed && a->wino_m != 2 && a->wino_m != 42) { set_error("bsvd_conv3x3: BSVD_F16: the Winograd form runs as F(2,3) only (wino_m 2 or 42), got wino_m %d", a->wino_m); return -24; }
    if (a->x_planar_ch > 0 && !a->head_w_packed) { set_error("bsvd_conv3x3: BSVD_F16: the unfused planar entry (x_planar_ch without head_w_packed) is not an MFMA layer; launch it as BSVD_F16X3"); return -24; }
    return 0;
}

// per-layer power-of-two weight scale (ABI v12): checked in front of every launch path; writes the three resolved factors
static int check_scales(const BsvdConvArgs *a, ConvParams *p)
{
    const struct { const char *nm; float v; float *dst; const void *pack; } sc[3] = {
        {"out_scale", a->out_scale, &p->out_scale, a->w_wino_packed ? a->w_wino_packed : a->w_packed},
        {"head_out_scale", a->head_out_scale, &p->head_out_scale, a->head_w_packed},
        {"pre_out_scale", a->pre_out_scale, &p->pre_out_scale, a->pre_w_packed}};
    for (const auto &s : sc) {
        if (!out_scale_ok(s.v, s.dst)) { set_error("bsvd_conv3x3: %s = %g must be 0 (= 1) or a finite, positive, normal power of two", s.nm, (double)s.v); return -23; }
        if (*s.dst == 1.0f) continue;
        if (!split_dtype(a->dtype)) { set_error("bsvd_conv3x3: %s = %g: the weight scale is an option of BSVD_F16X3", s.nm, (double)s.v); return -23; }
        if (!s.pack) { set_error("bsvd_conv3x3: %s = %g without the pack it belongs to", s.nm, (double)s.v); return -23; }
    }
    if (p->out_scale != 1.0f && a->w_wino_packed && a->wino_m >= 10 && a->wino_m < 20) { set_error("bsvd_conv3x3: out_scale is not available for wino_m %d (the all-positions-per-wave measurement kernel)", a->wino_m); return -23; }
    // the unfused planar entry runs head_kernel (conv3x3_edge_f32.hip) on an fp32 pack: it has no scale to undo
    if (p->out_scale != 1.0f && a->x_planar_ch > 0 && !a->head_w_packed) {
        set_error("bsvd_conv3x3: out_scale = %g is not available for the unfused planar entry (x_planar_ch without head_w_packed: an fp32 pack)", (double)p->out_scale); return -23;
    }
    return 0;
}

// every member of ConvParams but the three scales (check_scales) -- the modes' own fields at "off": check_v sets v_wg, check_pair pre_*,
// check_entry head_*, and the two fused kernels force vec_ok
static void fill_params(const BsvdConvArgs *a, ConvParams *p)
{
    p->x = (const float *)a->x;
    p->halo_prev = a->fold > 0 ? (const float *)a->halo_prev : nullptr;
    p->halo_next = a->fold > 0 ? (const float *)a->halo_next : nullptr;
    p->w = (const float *)(a->w_wino_packed ? a->w_wino_packed : a->w_packed);
    p->wino_m = a->w_wino_packed ? a->wino_m : 0;
    p->fat_min_wgs = a->fat_min_wgs > 0 ? a->fat_min_wgs : 0;
    p->bias = (const float *)a->bias_packed;
    p->extra = (const float *)a->extra;
    p->y = (float *)a->y;
    p->x_fs = a->x_frame_stride; p->extra_fs = a->extra_frame_stride; p->y_fs = a->y_frame_stride;
    p->halo_prev_ps = a->halo_prev_pstride; p->halo_prev_co = a->halo_prev_coff;
    p->halo_next_ps = a->halo_next_pstride; p->halo_next_co = a->halo_next_coff;
    p->extra_ps = a->extra_pstride; p->extra_cs = a->extra_cstride; p->resid_ch = a->resid_ch;
    p->fold = a->fold; p->frames = a->frames; p->H = a->H; p->W = a->W;
    p->Ho = (a->H - 1) / a->stride + 1; p->Wo = (a->W - 1) / a->stride + 1;
    p->Cin = a->Cin; p->Cout = a->Cout; p->act = a->act; p->epilogue = a->epilogue;
    p->ntx = p->nty = p->nct = 0;
    // 16-byte vector gather is legal when every 4-channel group has a single, aligned source
    bool vec = (a->fold & 3) == 0 && aligned16(a->x) && (a->x_frame_stride & 3) == 0;
    if (p->halo_prev) vec = vec && (a->halo_prev_pstride & 3) == 0 && (a->halo_prev_coff & 3) == 0 && aligned16(a->halo_prev);
    if (p->halo_next) vec = vec && (a->halo_next_pstride & 3) == 0 && (a->halo_next_coff & 3) == 0 && aligned16(a->halo_next);
    p->vec_ok = vec ? 1 : 0;
    p->one_pass = a->dtype == BSVD_F16 ? 1 : 0;
    p->flip = a->tile_order ? 1 : 0;
    p->prec = split_dtype(a->dtype) ? 1 : 0;
    p->extra_split = a->extra_split;
    p->y_planar_ch = a->y_planar_ch; p->y_clamp = a->y_clamp; p->y_lo = a->y_lo; p->y_hi = a->y_hi;
    p->head_w = nullptr; p->head_bias = nullptr; p->head_cin = 0;
    p->pre_w = nullptr; p->pre_bias = nullptr; p->pre_cin = 0; p->pre_act = 0;
    p->x_f32 = a->x_f32 ? 1 : 0; p->y_f32 = a->y_f32 ? 1 : 0;
    p->x_v = a->x_v; p->y_v = a->y_v; p->v_wg = 0;
}

// x_v / y_v: transformed-domain tensors of the Winograd form
static int check_v(const BsvdConvArgs *a, ConvParams *p)
{
    if (!a->x_v && !a->y_v) return 0;
    const int m = a->wino_m % 10;
    if (!split_dtype(a->dtype) || !a->w_wino_packed) { set_error("bsvd_conv3x3: x_v / y_v are options of the Winograd form (BSVD_F16X3 + w_wino_packed)"); return -22; }
    if ((a->x_v && a->x_v != m) || (a->y_v && a->y_v != m)) { set_error("bsvd_conv3x3: x_v / y_v (%d / %d) must be the form's m = %d", a->x_v, a->y_v, m); return -22; }
    if ((a->x_v && a->x_f32) || (a->y_v && a->y_f32)) { set_error("bsvd_conv3x3: a tensor is either plain fp32 or transformed, not both"); return -22; }
    if (a->y_v && a->epilogue != BSVD_EPI_PLAIN) { set_error("bsvd_conv3x3: y_v needs the PLAIN epilogue"); return -22; }
    if (a->x_v && a->fold > 0 && ((a->halo_prev && ((a->halo_prev_pstride & 15) || (a->halo_prev_coff & 15))) ||
                                  (a->halo_next && ((a->halo_next_pstride & 15) || (a->halo_next_coff & 15))))) {
        set_error("bsvd_conv3x3: x_v halos: pstride and coff are channel counts of transformed tensors (multiples of 16)"); return -22;
    }
    p->v_wg = v_groups(a->W, m);
    const int64_t vfe = v_plane_elems(a->H, a->W, a->x_v ? a->Cin : a->Cout, m);
    if (a->x_v && (a->frames > 1 && a->x_frame_stride < v_plane_elems(a->H, a->W, a->Cin, m))) { set_error("bsvd_conv3x3: x_v: x_frame_stride < the transformed frame"); return -22; }
    if (a->y_v && a->y_frame_stride < bsvd_v_frame_elems(a->H, a->W, a->Cout, m)) { set_error("bsvd_conv3x3: y_v: y_frame_stride < bsvd_v_frame_elems"); return -22; }
    if (!fits_2gib(vfe * 4)) { set_error("bsvd_conv3x3: transformed frame >= 2 GiB"); return -22; }
    return 0;
}

// x_f32 / y_f32: plain fp32 channels where the split mode carries fp16 pairs
static int check_f32(const BsvdConvArgs *a)
{
    if (a->x_f32 && !(split_dtype(a->dtype) && a->w_wino_packed)) { set_error("bsvd_conv3x3: x_f32 is the Winograd form's input option (BSVD_F16X3 + w_wino_packed)"); return -21; }
    if (a->y_f32 && (!split_dtype(a->dtype) || a->y_planar_ch > 0 || a->x_planar_ch > 0 || a->epilogue == BSVD_EPI_RESID || a->pre_w_packed || a->head_w_packed ||
                     (a->epilogue == BSVD_EPI_PS_ADD && !a->w_wino_packed))) {
        set_error("bsvd_conv3x3: y_f32 needs BSVD_F16X3 and a PLAIN NHWC layer (direct or Winograd form) or a PS_ADD layer of the Winograd form"); return -21;
    }
    return 0;
}

// Winograd form of a wide layer: explicit request, no silent fall-back to the direct kernel
static int check_wino(const BsvdConvArgs *a, const ConvParams &p, Route *r)
{
    if (a->x_planar_ch > 0 || a->head_w_packed) { set_error("bsvd_conv3x3: w_wino_packed: not with a planar / fused entry"); return -19; }
    if (const char *why = wino_unsupported(p, a->stride)) { set_error("bsvd_conv3x3: w_wino_packed (F(%d,3)): %s", a->wino_m, why); return -19; }
    // the all-positions-per-wave kernel (conv3x3_wino.hip, measurement builds) knows fp16 pairs only
    if (p.wino_m >= 10 && p.wino_m < 20 && (a->x_f32 || a->y_f32)) { set_error("bsvd_conv3x3: x_f32 / y_f32 are not available for wino_m %d", p.wino_m); return -21; }
    r->kind = ROUTE_WINO;
    return 0;
}

// fused pair of plain stride-1 convs: explicit request, never a silent two-launch fall-back
static int check_pair(const BsvdConvArgs *a, ConvParams *p, Route *r)
{
    if (a->dtype != BSVD_F16X3) { set_error("bsvd_conv3x3: the fused pair (pre_w_packed) is a BSVD_F16X3 kernel"); return -20; }
    if (a->x_planar_ch > 0 || a->head_w_packed) { set_error("bsvd_conv3x3: pre_w_packed: not with a planar input / fused entry"); return -20; }
    if (a->stride != 1 || a->fold != 0 || a->epilogue == BSVD_EPI_PS_ADD) { set_error("bsvd_conv3x3: fused pair needs stride 1, fold 0, PLAIN / RESID"); return -20; }
    // (Cin <= 64: the kernel carries TWO 32-channel pairs of the first conv's output -- pair 0 in the patch buffers, pair 1 in registers;
    //  a wider middle tensor would refill chunks 4.. with pair 1's data: refused, never silently wrong)
    if (a->pre_cin <= 0 || (a->pre_cin & 15) || (a->Cin & 31) || a->Cin > 64 || a->Cout > 64) {
        set_error("bsvd_conv3x3: fused pair needs pre_cin %% 16 == 0, Cin = 32 or 64, Cout <= 64 (pre_cin %d, Cin %d, Cout %d)", a->pre_cin, a->Cin, a->Cout); return -20;
    }
    if (a->pre_act < BSVD_ACT_NONE || a->pre_act > BSVD_ACT_RELU6) { set_error("bsvd_conv3x3: pre_act %d", a->pre_act); return -20; }
    if (!a->pre_bias || !aligned16(a->pre_w_packed) || !aligned16(a->pre_bias) || !aligned16(a->x) || (a->x_frame_stride & 3)) { set_error("bsvd_conv3x3: fused pair needs 16-byte aligned x, pre_w_packed and pre_bias"); return -20; }
    if (!fits_2gib((int64_t)a->H * a->W * (a->pre_cin > a->Cout ? a->pre_cin : a->Cout) * 4) || !fits_2gib((int64_t)a->pre_cin * 9 * a->Cin * 4)) {
        set_error("bsvd_conv3x3: frame / weights too large for the fused pair (2 GiB byte offsets)"); return -20;
    }
    if (a->y_planar_ch > 0 && (a->Cout != 16 || a->y_planar_ch > 4 || (a->epilogue == BSVD_EPI_RESID && a->resid_ch > a->y_planar_ch))) {
        set_error("bsvd_conv3x3: fused pair with a planar output needs Cout == 16 and 1..4 planar channels"); return -20;
    }
    p->pre_w = a->pre_w_packed; p->pre_bias = (const float *)a->pre_bias; p->pre_cin = a->pre_cin; p->pre_act = a->pre_act;
    p->vec_ok = 1;
    r->arg = 1;
    return 0;
}

// fused network entry: planar input -> (x_planar_ch -> Cin conv, act) -> (Cin -> Cout conv, act), one launch
static int check_entry(const BsvdConvArgs *a, ConvParams *p, Route *r)
{
    if (!split_dtype(a->dtype)) { set_error("bsvd_conv3x3: the fused entry (head_w_packed) is a BSVD_F16X3 kernel"); return -18; }
    if (a->x_planar_ch != 3 && a->x_planar_ch != 4) { set_error("bsvd_conv3x3: fused entry supports 3 or 4 planar input channels, got %d", a->x_planar_ch); return -18; }
    if ((a->Cin & 31) || a->Cout > 64 || a->epilogue != BSVD_EPI_PLAIN || a->y_planar_ch > 0) {
        set_error("bsvd_conv3x3: fused entry needs Cin %% 32 == 0, Cout <= 64 and the PLAIN epilogue (Cin %d, Cout %d)", a->Cin, a->Cout); return -18;
    }
    if (!a->head_bias || !aligned16(a->head_w_packed) || !aligned16(a->head_bias)) { set_error("bsvd_conv3x3: fused entry needs 16-byte aligned head_w_packed and head_bias"); return -18; }
    if (!fits_2gib((int64_t)a->H * a->W * a->Cout * 4)) { set_error("bsvd_conv3x3: frame too large for the fused entry"); return -18; }
    p->head_w = a->head_w_packed; p->head_bias = (const float *)a->head_bias; p->head_cin = a->x_planar_ch;
    p->vec_ok = 1;
    r->arg = 1;
    return 0;
}

// planar edge layers: the network's entry (fused, or the fp32 head kernel) and its exit (the MFMA kernel in split mode, else the fp32 tail kernel)
static int check_planar(const BsvdConvArgs *a, ConvParams *p, Route *r)
{
    if (a->x_planar_ch > 0 && a->y_planar_ch > 0) { set_error("bsvd_conv3x3: x_planar_ch and y_planar_ch are exclusive"); return -16; }
    if (a->stride != 1 || a->fold != 0) { set_error("bsvd_conv3x3: planar edge layers need stride 1 and fold 0"); return -16; }
    // (a count of elements, not of bytes: the edge kernels index floats with 32 bits)
    if (!fits_2gib((int64_t)a->H * a->W * (a->Cin > a->Cout ? a->Cin : a->Cout))) { set_error("bsvd_conv3x3: frame too large for the edge kernels"); return -16; }
    if (a->x_planar_ch > 0 && a->head_w_packed) return check_entry(a, p, r);
    if (a->x_planar_ch > 0) {
        if (a->Cin != 16 || a->epilogue != BSVD_EPI_PLAIN) { set_error("bsvd_conv3x3: planar input needs Cin == 16 (padded) and the PLAIN epilogue"); return -16; }
        *r = {ROUTE_HEAD_F32, a->x_planar_ch};
        return 0;
    }
    if (a->Cout != 16 || a->epilogue == BSVD_EPI_PS_ADD) { set_error("bsvd_conv3x3: planar output needs Cout == 16 (padded) and PLAIN/RESID"); return -16; }
    if (a->epilogue == BSVD_EPI_RESID && a->resid_ch > a->y_planar_ch) { set_error("bsvd_conv3x3: resid_ch > y_planar_ch"); return -16; }
    if (a->y_planar_ch > 4) { set_error("bsvd_conv3x3: planar output supports 1..4 channels, got %d", a->y_planar_ch); return -15; }
    // split16: the exit layer runs on the matrix cores too (one 32-channel column tile, 3-4 of them live; weights
    // split-packed like every other BSVD_F16X3 layer) and writes planar fp32 from its epilogue
    if (p->prec == 1) r->arg = 1;
    else *r = {ROUTE_TAIL_F32, a->y_planar_ch};
    return 0;
}

static int conv3x3_check(const BsvdConvArgs *a, ConvParams *p, Route *r)
{
    int rc;
    if ((rc = check_common(a)) || (rc = check_one_pass(a)) || (rc = check_scales(a, p))) return rc;
    fill_params(a, p);
    if ((rc = check_v(a, p)) || (rc = check_f32(a))) return rc;
    if (!aligned16(p->w)) { set_error("bsvd_conv3x3: w_packed / w_wino_packed must be 16-byte aligned"); return -13; }
    *r = {ROUTE_CONV, a->stride};
    if (a->w_wino_packed) return check_wino(a, *p, r);
    if (a->pre_w_packed) return check_pair(a, p, r);
    if (a->x_planar_ch > 0 || a->y_planar_ch > 0) return check_planar(a, p, r);
    return 0;
}

// name != nullptr: dry run, only writes the kernel instantiation that would be launched
static int conv3x3_impl(const BsvdConvArgs *a, void *stream, char *name, int name_len)
{
    ConvParams p;
    Route r;
    if (const int rc = conv3x3_check(a, &p, &r)) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (r.kind) {
    case ROUTE_WINO: return launch_winox(p, st, name, name_len);
    case ROUTE_HEAD_F32:
        if (name) { snprintf(name, name_len, "head_kernel<%d>%s", r.arg, p.prec == 1 ? "[f16x3 out]" : "[f32]"); return 0; }
        return launch_head_f32(p, r.arg, st);
    case ROUTE_TAIL_F32:
        if (name) { snprintf(name, name_len, "tail_kernel<%d>[f32]", r.arg == 3 ? 3 : 4); return 0; }
        return launch_tail_f32(p, r.arg, p.y_clamp, p.y_lo, p.y_hi, st);
    default: return launch_conv3x3(p, r.arg, st, name, name_len);
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

int bsvd_conv3x3(const BsvdConvArgs *a, void *stream) { return conv3x3_impl(a, stream, nullptr, 0); }

int bsvd_conv3x3_variant(const BsvdConvArgs *a, char *name, int32_t name_len)
{
    if (!name || name_len < 8) { set_error("bsvd_conv3x3_variant: name buffer too small"); return -1; }
    name[0] = 0;
    return conv3x3_impl(a, nullptr, name, name_len);
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
