/*
 * bsvd_hip.h -- C ABI of libbsvd_hip.so: the MI355X (gfx950) kernels behind the BSVD hot path.
 *
 * The reference has no FFI on this path: everything below BSVD.forward is torch ops
 * (/root/reference/Experimental_root/archs/bsvd_arch.py).  This header is the boundary the
 * MI355X engine puts in their place; each entry point names the reference op(s) it replaces.
 * The Python host (bsvd_amd/) binds it with ctypes; any other host binds it the same way
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / C++ types; no exceptions cross the ABI.
 *   - The library allocates nothing and keeps no global state besides a thread-local error string.
 *     Every buffer (activations, packed weights, halos) is owned and sized by the caller.
 *   - All work is enqueued asynchronously on the caller's HIP stream (pass it as void*, i.e. a
 *     hipStream_t; NULL = the default stream).  Calls on distinct streams may run concurrently.
 *   - Return value: 0 ok; <0 invalid argument (text via bsvd_last_error()); >0 a hipError_t.
 *   - Activations are NHWC ("channels last"): element (f, y, x, c) of a clip lives at
 *         base + f*frame_stride + (y*W + x)*C + c        (strides in ELEMENTS)
 *     with C already padded by the caller to a multiple of 16 (padded channels hold zeros).
 *   - Every stride is the caller's (tests/test_gpu_strides.py): a frame stride is >= the tight frame.  x_frame_stride takes any such value in
 *     BSVD_F32 (an unaligned x or stride runs the [generic] kernel); the NHWC x of BSVD_F16X3 and of the Winograd form, like its halos, needs
 *     16-byte aligned pointers and strides that are multiples of 4 elements, and anything else is refused (-17 / -19 / -20, naming the
 *     alignment) before a launch.  y and extra are the caller's to keep 16-byte aligned with strides that are multiples of 4 elements; the
 *     library does not check them.  No element outside [frames][H][W][C] of a tensor -- between its frames, in the other channels of a
 *     holding tensor -- influences a result; no byte outside y's logical elements is written; every logical element of y is written, padded
 *     channels included.
 *   - dtype: BSVD_F32 is the exact-fp32 mode (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain); BSVD_F16X3 the
 *     split-fp16 3-pass mode (see the enum).  In BSVD_F16X3 the edge layers convert: planar fp32 in -> split16,
 *     split16 -> planar fp32 out; the packed weights of MFMA layers are split16 too (bsvd_pack_weights dtype).
 *     BSVD_F16 is BSVD_F16X3's data contract with one MFMA pass, hi(w) * hi(x) (see the enum).
 */
// Arithmetic of BSVD_F32, bit for bit ("bitwise an fmaf chain" above, spelled out; the CPU model oracle/chain_ref.c restates it,
// tests/test_gpu_fp32_chain.py compares the bits on the MI355X, profiles/fp32_chain_bits.txt is the record).  Per output value, with x the
// gathered input of the frame -- zero outside the image and in its padded channels -- and every operation below ONE fp32 operation, round to
// nearest even:
//   chain     acc = fmaf(x, w, acc) once per term, in the kernel's order.  A term with a zero operand changes nothing but the sign of a zero
//             accumulator and may be skipped: results are the chain's up to the sign of zero.
//     MFMA layers -- everything but the two planar edge layers; FAST, [generic] and [fold8] alike, every tile, both tile_order values:
//             acc starts at +0; for each 16-channel chunk c, for each tap t = 3 ky + kx, for g in 0..1, for j in 0..3:
//             channel 16c + 8g + j, then channel 16c + 8g + 4 + j (the two k of one v_mfma_f32_32x32x2_f32, k = 0 first).
//     planar exit  (y_planar_ch > 0): acc starts at +0; for each chunk c, each tap t, channel 16c + 0 .. 16c + 15.
//     planar entry (x_planar_ch > 0): acc starts at the BIAS (+0 without one); for each tap t, channel 0 .. x_planar_ch - 1.
//   bias      v = acc + bias, one rounding (== fmaf(acc, 1.0f, bias)); the planar entry has it at the chain's start instead.
//   act       BSVD_ACT_RELU max(v, 0); BSVD_ACT_RELU6 min(max(v, 0), 6).
//   epilogue  PS_ADD v + skip; RESID extra - v on the first resid_ch channels; then, with y_clamp, min(max(v, y_lo), y_hi).
// A schedule, shard or halo form changes which launch computes a value, never its chain: clip, stream and sharded runs give the same bits.
#ifndef BSVD_HIP_H
#define BSVD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSVD_ABI_VERSION 12

/* dtype.  BSVD_F32: exact fp32 (v_mfma_f32_32x32x2_f32).  BSVD_F16X3 ("split16"): every fp32 value v is carried as
 * an fp16 pair hi = fp16(v), lo = fp16(v - hi); a 16-channel chunk of a pixel is stored as [hi x16 | lo x16] in the
 * same 64 bytes the fp32 layout uses (so shapes, strides and halo offsets are identical), and each K = 16 block is
 * three fp16 MFMAs (hi*hi + lo*hi + hi*lo, fp32 accumulate).  fp32-class accuracy (2-4e-5 max-abs on bsvd_c64) at
 * several times the fp32-MFMA rate.
 *
 * BSVD_F16: the BSVD_F16X3 data contract with ONE MFMA pass.  Tensors, halos, strides, rings and weight packs are byte for byte
 * BSVD_F16X3's -- an F16X3 pack (bsvd_pack_weights / bsvd_pack_weights_wino with wino_m = 2 / bsvd_pack_head_weights) serves BOTH modes;
 * there is no BSVD_F16 pack and the pack entry points refuse the value.  Each K = 16 block is one fp16 MFMA, hi(w) * hi(x) with
 * hi = fp16(v) (Winograd form: the hi of each transformed value's pair), fp32 accumulate; the lo halves of weights and activations are
 * never fetched as MFMA operands and no result depends on them.  Behind the accumulator nothing changes: fmaf(acc, out_scale, bias),
 * activation, PS_ADD / RESID / clamp in fp32 with the skip / residual operands decoded from FULL pairs, the result stored as the
 * canonical pair (or plain fp32 for y_f32, planar fp32 at the exit).  fp16-class accuracy: operands rounded to 11 bits (the reference's
 * own GPU arithmetic is fp16 autocast); it misses the 1e-3 parity bar of the other two modes and is never chosen automatically.
 * Kernels: every direct-form split tile, the fused entry (head_w_packed) and the F(2,3) Winograd form (wino_m 2 / 42; x_f32 / y_f32 /
 * PS_ADD included).  Refused with -24 before any launch: pre_w_packed, x_v / y_v, any other wino_m, and the unfused planar entry
 * (x_planar_ch without head_w_packed: an fp32 VALU kernel, launched as BSVD_F16X3).  The BSVD_F16X3 refusals apply unchanged.
 *
 * Numbering.  The value 1 was reserved for a plain-fp16 mode with fp16 STORAGE and stays retired: every library up to and including
 * this one answers -2 to it (the recorded validation answers pin that).  BSVD_F16 is 3, added without a new BSVD_ABI_VERSION -- the
 * struct is unchanged; discover the mode with bsvd_conv3x3_variant (-2 from a library that lacks it, else a name with "[f16]"). */
// "fp32-class" holds for weights around init scale.  lo is an fp16 SUBNORMAL for |v| < 2^-3 (kept by conversions and MFMAs, asserted in
// tests/test_gpu_range.py), so a pair resolves 2^-24 absolute whatever its size and a layer's relative error is about 2.6e-8 / std(w):
// 6e-7 at std 0.03, 1e-5 at 2^-4 of that, 1e-4 at 2^-8, plain-fp16 class (2e-3) at 2^-12; a stored output resolves 2^-25 absolute.
// DESIGN.md 4.1b has the table measured on the MI355X.  The remedy is the per-layer power-of-two weight scale, BsvdConvArgs.out_scale (ABI v12).
enum { BSVD_F32 = 0, /* 1: retired, refused */ BSVD_F16X3 = 2, BSVD_F16 = 3 };
enum { BSVD_ACT_NONE = 0, BSVD_ACT_RELU = 1, BSVD_ACT_RELU6 = 2 }; /* get_act_function, bsvd_arch.py:185-192 */
enum {
    BSVD_EPI_PLAIN = 0,   /* y = act(conv + bias)                                                     */
    BSVD_EPI_PS_ADD = 1,  /* nn.PixelShuffle(2) (+ skip add): UpBlock :265-266 + DenBlock.none_add :402 */
    BSVD_EPI_RESID = 2    /* y[:resid_ch] = extra[:resid_ch] - y[:resid_ch]: DenBlock.none_minus :408-414 */
};

/*
 * One fused layer over a whole clip (or a single frame in streaming mode):
 *
 *     y[f] = epilogue( act( conv3x3( gather(x[f-1], x[f], x[f+1], fold), w, stride, pad 1 ) + bias ) )
 *
 * Replaces, per call: nn.Conv2d 3x3 (bsvd_arch.py:31-38, 208-213, 238, 265, 295-298), the
 * torch.cat temporal-shift gather of ShiftConv.forward (:42-50), the zero tensors BiBufferConv makes
 * at stream start/end (:94, :104), nn.ReLU6/ReLU (:185-192), nn.PixelShuffle(2) (:266), the skip add
 * (:402-406) and the residual (:408-414).
 *
 * Temporal-shift gather (fold > 0): input channel c of frame f is read from
 *     frame f+1  if c <  fold            (for f == frames-1: from halo_next, zeros if NULL)
 *     frame f-1  if fold <= c < 2*fold   (for f == 0:        from halo_prev, zeros if NULL)
 *     frame f    otherwise.
 * Halo element (pixel p, channel c) is read at
 *     halo_prev[p*halo_prev_pstride + halo_prev_coff + (c - fold)],
 *     halo_next[p*halo_next_pstride + halo_next_coff + c].
 * (compact [H][W][fold] slice: pstride = fold, coff = 0; a full NHWC frame: pstride = Cin,
 *  coff = fold resp. 0.)  This is what a neighbouring frame-window shard sends over RCCL, and in
 *  streaming mode it is BiBufferConv's left_fold_2fold / input_right.
 * BSVD_F16X3 with fold 8 (half a 16-channel chunk of fp16 pairs per source) knows two halo shapes: the compact slice of bsvd_halo_pack
 * (pstride 8: [hi x8 | lo x8]) and the slice in its place inside a split16 frame (pstride % 16 == 0).  There coff names the CHUNK -- coff -
 * coff % 16 is the first channel of the frame's chunk 0 inside a (possibly wider) holding tensor -- and the slice's place inside the chunk is
 * fixed: its second half for halo_prev, its first for halo_next; coff % 16 is ignored (a neighbour frame is passed with coff = fold resp. 0).
 * A pstride that is neither, or a chunk that does not lie inside the pixel (coff - coff % 16 + 16 > pstride), returns -17.
 */
// Channel counts: every multiple of 16 is served in every dtype, not only the powers of two of the shipped
// networks (measured at the widths between them: profiles/channel_widths.txt).  Refused: a Cin or Cout that
// is no positive multiple of 16 (-5); PS_ADD with Cout % 64 != 0 (-10); in the split dtypes a fold that is
// neither a multiple of 16 nor 8 with Cout <= 64 (-17); w_wino_packed with Cout % 32 != 0 or fold % 16 != 0 (-19).
typedef struct BsvdConvArgs {
    const void *x;              /* [frames][H][W][Cin]                                              */
    int64_t x_frame_stride;     /* elements between consecutive frames of x                          */
    const void *halo_prev;      /* nullable */
    const void *halo_next;      /* nullable */
    int32_t halo_prev_pstride, halo_prev_coff;
    int32_t halo_next_pstride, halo_next_coff;
    int32_t fold;               /* 0 = plain conv (no temporal shift)                                */
    const void *w_packed;       /* from bsvd_pack_weights()                                          */
    const void *bias_packed;    /* [Cout] from bsvd_pack_weights(); nullable                         */
    const void *extra;          /* PS_ADD: skip tensor laid out like y (nullable); RESID: base tensor */
    int64_t extra_frame_stride;
    int32_t extra_pstride;      /* elements between pixels of extra                                  */
    int32_t extra_cstride;      /* elements between channels of extra                                */
    int32_t resid_ch;           /* RESID: number of leading channels replaced (3 in the reference)   */
    void *y;                    /* PLAIN/RESID: [frames][Ho][Wo][Cout]; PS_ADD: [frames][2Ho][2Wo][Cout/4] */
    int64_t y_frame_stride;
    int32_t frames, H, W;       /* input spatial size; Ho = (H-1)/stride + 1                          */
    int32_t Cin, Cout;          /* padded channel counts: Cin % 16 == 0, Cout % 16 == 0 (PS_ADD: Cout % 64 == 0) */
    int32_t stride;             /* 1 or 2                                                            */
    int32_t act, epilogue, dtype;
    /* Clip entry/exit fused into the edge layers (optional; 0 = plain NHWC as described above):
     *   x_planar_ch > 0: x is the caller's planar tensor [frames][x_planar_ch][H][W] fp32 (3 or 4 channels,
     *                    BSVD.forward's reshaped input, bsvd_arch.py:494-499); needs Cin == 16, stride 1, fold 0, PLAIN.
     *   y_planar_ch > 0: y is planar [frames][y_planar_ch][H][W] fp32 (1..4 channels, the tensor torch.cat(out_seq)
     *                    returns, :552); needs Cout == 16, stride 1, fold 0, PLAIN or RESID; y_clamp != 0 additionally
     *                    clamps to [y_lo, y_hi] (the callers' torch.clamp, validation_seq_infer.py:24).
     * Weights of these two layers: the planar-INPUT layer always takes an fp32 pack (bsvd_pack_weights dtype BSVD_F32; it
     * runs on a VALU kernel and, in BSVD_F16X3, writes split16).  The planar-OUTPUT layer takes the pack of its dtype: in
     * BSVD_F16X3 it is an MFMA layer like any other (split-packed weights, split16 input). */
    int32_t x_planar_ch, y_planar_ch, y_clamp;
    float y_lo, y_hi;
    int32_t extra_split;        /* BSVD_F16X3 + y_planar_ch: the RESID base `extra` is a split16 NHWC tensor (extra_pstride
                                 * floats per pixel) instead of fp32 with generic strides                              */
    int32_t tile_order;         /* 0: workgroups walk the output tiles first frame / first row first; 1: in reverse.  Results
                                 * are identical; a layer-major host alternates it layer by layer so that every layer starts with
                                 * the part of its input the previous layer wrote LAST -- still in the 256 MiB Infinity Cache when
                                 * the clip's tensors (0.3-1.3 GB) are not (+0.3 % on the 10-frame 540x960 clip)          */
    /* Fused network entry (ABI v8, BSVD_F16X3 only): InputCvBlock's two convs (bsvd_arch.py:207-216) in ONE launch.
     * With x_planar_ch > 0 AND head_w_packed != NULL, x is the caller's planar tensor [frames][x_planar_ch][H][W] fp32 (3 or 4
     * channels) and the kernel computes  t = act(conv3x3(x, head_w) + head_bias)  (x_planar_ch -> Cin channels, zero outside
     * the image) on every tile's 18 x 18 patch itself -- on the matrix cores, K = 36 padded to 48, straight into the LDS
     * patch of the main conv -- and then  y = epilogue(act(conv3x3(t, w_packed) + bias)).  The Cin-channel tensor t never
     * exists in HBM (1.33 GB written + read per 10-frame 540x960 clip).  Needs Cin % 32 == 0, Cout <= 64, stride 1, fold 0,
     * BSVD_EPI_PLAIN; both convs share `act`.  head_w_packed: bsvd_pack_head_weights(); head_bias: [Cin] fp32. */
    const void *head_w_packed;
    const void *head_bias;
    /* Winograd form of a wide layer (ABI v9, BSVD_F16X3 only).  w_wino_packed != NULL selects the 1-D Winograd F(wino_m, 3)
     * kernel (conv3x3_winox.hip, one transformed position per wave) with the TRANSFORMED weights of bsvd_pack_weights_wino();
     * w_packed is then ignored (may be NULL).  wino_m:
     *    2 | 6    F(2,3) | F(6,3).  The kernel picks its half-height pixel tile for grids that do not fill the chip (single-frame
     *             launches); both tiles compute every output with the same instruction sequence (bit-identical).  On the 16-row
     *             tile grid a last row band with <= 8 live rows (Ho mod 16 in 1 .. 8) is walked two tiles per workgroup (F(2,3):
     *             folded tiles) or on the 8-row body (F(6,3)) -- again the same instruction sequence per output.
     *   42 | 46   the same two forms, never on the half-height tile: for launches that run beside another stream's or graph
     *             branch's kernels (idle CUs are not idle there).  Same bits as 2 | 6.
     *   Other codes (F(4,3), forced tiles, 4-wave workgroups, the persistent form, the all-positions-per-wave kernel) exist in
     *   MEASUREMENT builds of the library only (-DBSVD_MEASURE: bsvd_build_info() & BSVD_BUILD_MEASURE; tools/build_measure.sh);
     *   the product library answers them with -19.
     * Same contract and tensors as the direct form -- gather, halos, bias, activation, PLAIN / PS_ADD epilogues -- but 6 (F(2,3)) or
     * 4 (F(6,3)) instead of 9 tap-GEMMs per output pixel; results differ from the direct form in the last bits (fp32 transforms,
     * both inside the same error class: 5e-5 max-abs on bsvd_c64), so a host must use ONE form per layer in every schedule it wants
     * bit-identical (clip / stream / sharded).  Needs stride 1, fold % 16 == 0, Cout % 32 == 0, 16-byte aligned x / halo pointers
     * and strides, H*W*Cin*4 and H*W*halo_pstride*4 < 2 GiB, no planar / fused-entry / RESID options; anything else returns -19
     * with the reason -- never a silent direct launch.
     * fp16 range: the kernel converts TRANSFORMED activations (sums of up to 2x / 4.7x the inputs for F(2,3) / F(6,3)) with
     * saturating conversions (MODE.FP16_OVFL): unchanged below 65504, a pair still carries a transformed value up to 131008 (at
     * reduced precision, relative 2^-13) and saturates beyond; finite inputs never produce inf / NaN.  Weights: bsvd_pack_weights_wino saturates U = G g at +-65504; a host should keep a
     * layer whose max |w| x (largest |G| row sum: 1.5 / 15.04) leaves fp16's range on the direct form (bsvd_amd.engine does). */
    const void *w_wino_packed;
    int32_t wino_m;
    /* Tuning (ABI v9; 0 = the library's measured default, 800): the smallest grid, in 256-px x 128-channel workgroups, for which a
     * wide direct-form BSVD_F16X3 layer takes the 128-accumulator tile instead of the 64-accumulator one.  Both tiles compute the
     * same bits; the field replaces an environment variable the library used to read once per process. */
    int32_t fat_min_wgs;
    /* Fused pair of plain stride-1 convs (ABI v10, BSVD_F16X3 only): with pre_w_packed != NULL the launch computes
     *     t = pre_act(conv3x3(x, pre_w) + pre_bias)            (pre_cin -> Cin channels, zero outside the image)
     *     y = epilogue(act(conv3x3(t, w_packed) + bias))       (Cin -> Cout channels; PLAIN, RESID or the planar exit)
     * in ONE kernel: every tile computes the first conv on its own 18 x 18 patch (full K = 9 pre_cin on the matrix cores, the input
     * patch staged chunk by chunk through LDS) a pair of 16-channel chunks at a time, straight into the LDS patch of the second
     * conv; the Cin-channel tensor t never exists in HBM (1.33 GB written + read per 10-frame 540x960 clip at 64 channels).  The
     * price is the halo: 324 patch pixels on 12 MFMA row-tile slots per 256 output pixels = 1.5x the first conv's MFMAs -- on the
     * MI355X the pair is 11-13 % SLOWER than the two launches while moving half their HBM bytes: a choice for
     * hosts short of bandwidth, not of matrix time.  x is the first
     * conv's NHWC input [frames][H][W][pre_cin] (x_frame_stride its frame stride); pre_w_packed = bsvd_pack_weights(dtype
     * BSVD_F16X3) of the first conv (pre_cin -> Cin), pre_bias its bias_packed [Cin].  Both convs: OutputCvBlock / InputCvBlock,
     * bsvd_arch.py:194-226, 287-306.  Needs pre_cin % 16 == 0, Cin = 32 or 64 (the kernel carries two 32-channel pairs of t), Cout <= 64, stride 1, fold 0, no planar INPUT, no
     * head_w_packed / w_wino_packed; anything else returns -20 with the reason.  Per output the arithmetic of both convs is the
     * stand-alone kernels': fused == unfused bit for bit. */
    const void *pre_w_packed;
    const void *pre_bias;
    int32_t pre_cin, pre_act;
    /* Plain-fp32 hand-over between split-mode layers (ABI v10, BSVD_F16X3 only).  A tensor that only Winograd-form layers read need
     * not be carried as fp16 pairs: its producer stores the fp32 value itself (y_f32 != 0: PLAIN layers of the direct kernel, PLAIN and
     * PS_ADD layers of the Winograd kernel; same [frames][H][W][C] shape, strides and bytes: 4 per value either way) and its consumer
     * reads it as such (x_f32 != 0, with w_wino_packed only: x AND both halos hold fp32 channels).  The consumer's input transform then
     * starts from the value -- no decode, one 8-byte load per position, the transform on channel pairs -- which takes about a fifth off
     * the transform's instructions; values are exact fp32 instead of 22-bit pairs.  Anything else returns -21. */
    int32_t x_f32, y_f32;
    /* Transformed-domain hand-over between Winograd-form layers (ABI v11, BSVD_F16X3 + w_wino_packed only).  The input
     * transform of F(m,3) -- V = BT d over the m + 2 pixels of a group, re-split into fp16 pairs -- is a property of the TENSOR, not of its
     * reader: done in the reader's K loop it is repeated per output-channel tile and its VALU time adds to the MFMA time of the SIMD it
     * shares.  With y_v != 0 the producer's epilogue does it ONCE, on the fp32 values it holds anyway, and stores the
     * tensor in the transformed domain; with x_v != 0 the reader's K loop is a plain 16-byte copy into LDS.  Layout of such a tensor, per
     * frame (bsvd_v_frame_elems(H, W, C, m) floats):
     *     B[row][T tiles of 8 groups][C / 16 chunks] blocks of (m + 2) x 512 + 128 bytes (4224 for F(6,3)):
     *         [m + 2 positions][4 quarters: hi c0-7, hi c8-15, lo c0-7, lo c8-15][8 groups] x 16 bytes -- the reader's LDS planes of one patch row of
     *         one chunk, contiguous; a group = m consecutive pixels of a row, T = ceil(W / 8m); position xi of group g =
     *         sum_i BT[xi][i] * d[m g - 1 + i], pixels outside the image = 0 -- followed by the block's EDGE LINE [side 0 | 1][4 quarters] x 16
     *         bytes: position 0 of the tile's first group (side 0) and position m + 1 of its last group (side 1), the two values of a tile row
     *         that need a pixel of the NEIGHBOURING tile.  Readers take these two values from the edge line, never from the planes;
     *     E[row][T][4][C] fp32 behind the blocks -- the producer's edge record (partial sums of those two positions + the tile's own first / last
     *         pixel column), consumed by the patch pass that bsvd_conv3x3 issues right behind a y_v launch on the same stream (one small
     *         second kernel that fills the edge lines: the only cross-tile dependency of the transform).
     * x_v / y_v carry the form's m (2, 4 or 6) and must equal wino_m % 10 of the layer (x_v) resp. of the tensor's reader (y_v).
     * x_v: x AND both halos are such tensors -- halo_*_pstride = channels of the holding tensor, halo_*_coff = first channel, both
     * multiples of 16, exactly as for NHWC halos; x_frame_stride = elements between frames (>= bsvd_v_frame_elems).
     * y_v: PLAIN layers of the Winograd kernel whose own form has the same m (the epilogue's pixel groups are the reader's groups);
     * y_frame_stride likewise.  Not with x_f32 / y_f32 on the same tensor.  Anything else returns -22. */
    int32_t x_v, y_v;
    /* Per-layer power-of-two weight scale (ABI v12, BSVD_F16X3 only).  A weight pair resolves 2^-24 ABSOLUTE (lo is an
     * fp16 subnormal for |w| < 2^-3), so a layer of small weights loses relative precision, and one of weights beyond 65504 cannot be
     * packed at all.  The remedy is the caller's: pack 2^e w -- with the unchanged bsvd_pack_weights / bsvd_pack_weights_wino /
     * bsvd_pack_head_weights; a power-of-two multiple of w is exact in fp32 and G (2^e g) = 2^e G g -- with e chosen so that the layer's
     * weights sit where a pair has its 22 bits, pass the bias UNSCALED and out_scale = 2^-e.  Every split-mode epilogue computes
     *     fmaf(acc, out_scale, bias)
     * in place of acc + bias: one rounding of the exact (acc 2^-e) + bias (barring underflow of acc 2^-e), bit-identical to acc + bias for
     * out_scale = 1, the same instruction count.  One kernel-uniform factor per conv, never per channel:
     *   out_scale       the main conv (w_packed / w_wino_packed);
     *   head_out_scale  the fused entry's first conv (head_w_packed);
     *   pre_out_scale   the fused pair's first conv (pre_w_packed).
     * 0.0f means 1.0 (zeroed structs of older callers).  Any other value must be a finite, positive, normal, exact power of two; a value
     * != 1 additionally needs dtype BSVD_F16X3, head_ / pre_out_scale their pack, and a wino_m code other than the all-positions-per-wave
     * measurement kernel's (12); out_scale != 1 is refused for the UNFUSED planar entry (x_planar_ch without head_w_packed), whose pack
     * is plain fp32.  Anything else returns -23 with the reason. */
    float out_scale, head_out_scale, pre_out_scale;
} BsvdConvArgs;

int bsvd_abi_version(void);
int bsvd_conv_args_size(void);   /* sizeof(BsvdConvArgs) as compiled into the library (binding sanity check) */
/* ABI v10: bit set of how this library was built.  BSVD_BUILD_MEASURE: a measurement build (-DBSVD_MEASURE) that also contains
 * the kernel variants DESIGN.md 4.1d records as slower (more wino_m codes); the product library returns 0. */
#define BSVD_BUILD_MEASURE 1
int bsvd_build_info(void);
const char *bsvd_last_error(void);

/* Transformed-domain tensors (BsvdConvArgs.x_v / y_v): floats per frame (V planes + edge record), groups per row, and a stand-alone
 * transform of an NHWC tensor (x_f32 != 0: plain fp32 channels, else fp16 pairs) into that layout -- what a y_v producer writes, computed
 * directly (no edge record needed; the E block is zero-filled).  Test / measurement aid and the fallback for a producer that cannot
 * write the layout itself.  m = 2, 4 or 6; C % 16 == 0.  Writes the bsvd_v_frame_elems floats of every frame, nothing between frames. */
int64_t bsvd_v_frame_elems(int32_t H, int32_t W, int32_t C, int32_t m);
int32_t bsvd_v_groups(int32_t W, int32_t m);
int bsvd_to_v(const void *x, int64_t x_frame_stride, int32_t x_f32, void *v, int64_t v_frame_stride, int32_t frames, int32_t H, int32_t W,
              int32_t C, int32_t m, void *stream);

/* The fused layer above (BSVD_F32: exact fp32 MFMA; BSVD_F16X3: split-fp16 3-pass MFMA). */
int bsvd_conv3x3(const BsvdConvArgs *args, void *stream);

/* Dry run: validates args exactly like bsvd_conv3x3 and writes the name of the kernel instantiation it would launch
 * (e.g. "conv3x3_kernel<4,2,2,2,1>[f16x3]" = <MT,NT,WM,WN,STRIDE>) -- profiling aid, launches nothing. */
int bsvd_conv3x3_variant(const BsvdConvArgs *args, char *name, int32_t name_len);

/*
 * Re-orders one nn.Conv2d weight [Cout][Cin][3][3] (+ bias [Cout]) into the layout bsvd_conv3x3
 * streams through LDS: w_packed[Cin_pad/16][9][4][Cout_pad][4] (the last index runs over 4
 * consecutive input channels), zero-filled padding.  pixel_shuffle != 0 additionally permutes the
 * output channels so that the four PixelShuffle sub-pixels become four contiguous channel groups:
 *   packed column sub*(Cout_pad/4) + c   <-   original output channel 4*c + sub.
 * Sizes: w_packed needs bsvd_packed_weight_elems(Cin_pad, Cout_pad) elements, bias_packed Cout_pad.
 * (One-time transform of the tensors BSVD.load() produces, bsvd_arch.py:462-474.)
 */
int64_t bsvd_packed_weight_elems(int32_t Cin_pad, int32_t Cout_pad);
int bsvd_pack_weights(const float *w_oihw, const float *bias, int32_t Cin, int32_t Cout,
                      int32_t Cin_pad, int32_t Cout_pad, int32_t pixel_shuffle, int32_t dtype,
                      void *w_packed, void *bias_packed, void *stream);

/*
 * Weights of the Winograd form (BsvdConvArgs.w_wino_packed): U[xi][ky] = sum_kx G[xi][kx] * w[.][.][ky][kx] for the
 * m + 2 transformed positions xi of F(m, 3), m = 2 | 4 | 6 (bsvd_amd/csrc/wino_forms.h), computed in double precision, split into fp16
 * pairs and laid out [Cin_pad/16][m + 2][3][hi, lo][2][Cout_pad][8 fp16]; pixel_shuffle permutes the output channels like
 * bsvd_pack_weights.  w_packed needs bsvd_packed_wino_weight_elems(Cin_pad, Cout_pad, m) 4-byte elements; bias_packed
 * (nullable) [Cout_pad] fp32 as in bsvd_pack_weights.
 */
int64_t bsvd_packed_wino_weight_elems(int32_t Cin_pad, int32_t Cout_pad, int32_t m);
int bsvd_pack_weights_wino(const float *w_oihw, const float *bias, int32_t Cin, int32_t Cout, int32_t Cin_pad,
                           int32_t Cout_pad, int32_t pixel_shuffle, int32_t m, void *w_packed, void *bias_packed,
                           void *stream);

/*
 * Weights of the fused network entry (BsvdConvArgs.head_w_packed): the first conv's [Cmid][Cin][3][3] (Cin = 3 or 4) as the
 * A operand of v_mfma_f32_32x32x16_f16 -- [Cmid_pad/32 channel pairs][3 k-steps][64 lanes][hi x8 | lo x8] fp16 with
 * k = tap*4 + channel (36 real of 48) -- plus head_bias[Cmid_pad] fp32 (zero padded).  w_packed needs
 * bsvd_packed_head_weight_bytes(Cmid_pad) bytes.
 */
int64_t bsvd_packed_head_weight_bytes(int32_t Cmid_pad);
int bsvd_pack_head_weights(const float *w_oihw, const float *bias, int32_t Cin, int32_t Cmid, int32_t Cmid_pad,
                           void *w_packed, float *bias_packed, void *stream);

/*
 * Clip entry/exit: the reference feeds NCHW tensors (BSVD.forward reshape, bsvd_arch.py:494-499,
 * and torch.cat(out_seq_clip) :552); callers then clamp to [0,1] (validation_seq_infer.py:24).
 *   nchw_to_nhwc: src [frames][C][H][W] fp32  ->  dst [frames][H][W][C_pad] (zero padded channels)
 *   nhwc_to_nchw: src [frames][H][W][C_pad]   ->  dst [frames][C][H][W] fp32, optional clamp to [lo,hi]
 */
int bsvd_nchw_to_nhwc(const float *src, void *dst, int32_t frames, int32_t C, int32_t H, int32_t W,
                      int32_t C_pad, int32_t dtype, void *stream);
int bsvd_nhwc_to_nchw(const void *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W,
                      int32_t C_pad, int32_t dtype, int32_t do_clamp, float lo, float hi, void *stream);

/*
 * uint8 frame I/O on device (the reference normalises on the host, utils_common.py:184, and rounds
 * with tensor2img, img_util.py:66,87-90).  u8_to_planar: src uint8 [frames][H][W][C] (src_hwc != 0) or
 * [frames][C][H][W] -> dst planar fp32 [frames][C + const_channels][H][W] = src/255 with `const_channels` trailing
 * channels filled with const_val (the constant sigma map of temp_denoise, validation_seq_infer.py:19-21).
 * planar_to_u8: src planar fp32 [frames][C][H][W] -> clamp to [0,1], x255, round half to even -> uint8, HWC or planar,
 * optionally with the channel order reversed (RGB -> BGR like tensor2img).
 */
int bsvd_u8_to_planar(const uint8_t *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t src_hwc,
                      int32_t const_channels, float const_val, void *stream);
int bsvd_planar_to_u8(const float *src, uint8_t *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t dst_hwc,
                      int32_t reverse_channels, void *stream);

/*
 * YUV 4:2:0 frame I/O on device: NV12 (8 bit) and P010 (10 bit) surfaces, as decoders, capture cards and encoders hand them over, in place
 * of the packed RGB above.  The reference has no YUV path: it builds the network input from RGB frames (validation_seq_infer.py:15-24,
 * what yuv420_to_planar stands in for together with the colour conversion a caller would do on the host) and makes the output image with
 * tensor2img (img_util.py:66,87-90, what planar_to_yuv420 stands in for).  Added without a new BSVD_ABI_VERSION: discover the three
 * entry points by symbol (dlsym); a version-12 library without them has no YUV path.
 *
 * Surface, per frame: a Y plane of H rows directly followed by an interleaved CbCr plane of H/2 rows, both with row_pitch BYTES per row;
 * frames frame_stride bytes apart.  NV12: one byte per sample.  P010: one little-endian 16-bit word per sample, the 10-bit code in the
 * high bits (code = word >> 6 in, word = code << 6 out; the low 6 bits are ignored in, zero out).  H and W are multiples of 4; bytes of a
 * row beyond W samples are never read and never written.  With b = 8 | 10 bits and s = 2^(b-8):
 *   matrix      (Kr, Kb) = BT.601 (0.299, 0.114) | BT.709 (0.2126, 0.0722) | BT.2020 non-constant-luminance (0.2627, 0.0593), Kg = 1 - Kr - Kb
 *   range       limited: y = (Y - 16s) / 219s, c = (C - 128s) / 224s;  full: y = Y / (2^b - 1), c = (C - 2^(b-1)) / (2^b - 1)
 *   chroma      NEAREST: a 2x2 luma block shares its chroma sample (in) / takes the mean of the block (out).  LINEAR: chroma sample (i, j)
 *               sits at luma (2i, 2j + 0.5), the MPEG-2 / H.264 / HEVC default siting.  In: rows 2j, 2j+1 take c[j-1]/4 + 3c[j]/4,
 *               3c[j]/4 + c[j+1]/4, then even columns c[i], odd columns (c[i] + c[i+1])/2, indices clamped at the frame edges.  Out: the
 *               mean of the two rows, then [1 2 1]/4 over columns 2i-1, 2i, 2i+1, edge-clamped.
 * yuv420_to_planar: dst planar fp32 [frames][3 + const_channels][H][W] (the tensor of bsvd_u8_to_planar, trailing channels = const_value):
 *   R = y + 2(1-Kr) cr, B = y + 2(1-Kb) cb, G = y - (2Kr(1-Kr)/Kg) cr - (2Kb(1-Kb)/Kg) cb.  NOT clamped: the out-of-gamut values of a
 *   noisy source are information for a denoiser.
 * planar_to_yuv420: src planar fp32 [frames][3][H][W]: R, G, B clamped to [0,1], Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / 2(1-Kb),
 *   Cr = (R - Y') / 2(1-Kr), chroma filter, scale to codes, clamp to the legal range (limited: luma [16s, 235s], chroma [16s, 240s]; full:
 *   [0, 2^b - 1]), round half to even.
 * Both return -3, naming the argument in bsvd_last_error(), for: a NULL pointer; frames <= 0; H or W <= 0 or not a multiple of 4; an unknown
 * enum value; reserved != 0; row_pitch below W samples; with P010 a row_pitch / frame_stride that is not a multiple of 2 or a surface
 * pointer that is not 2-byte aligned; frame_stride below one frame; a planar pointer that is not 16-byte aligned; const_channels < 0.
 * bsvd_yuv420_frame_bytes: row_pitch * H * 3 / 2 (row_pitch 0 = tight), -1 on bad arguments.
 */
enum { BSVD_PIX_NV12 = 0, BSVD_PIX_P010 = 1 };
enum { BSVD_MATRIX_BT601 = 0, BSVD_MATRIX_BT709 = 1, BSVD_MATRIX_BT2020 = 2 };
enum { BSVD_CHROMA_NEAREST = 0, BSVD_CHROMA_LINEAR = 1 };
typedef struct BsvdYuvDesc {
    int32_t pix_fmt, matrix, full_range, chroma;
    int32_t row_pitch;      /* bytes; 0 = tight (W samples) */
    int32_t reserved;       /* must be 0 */
    int64_t frame_stride;   /* bytes; 0 = tight (row_pitch * H * 3 / 2) */
} BsvdYuvDesc;
int64_t bsvd_yuv420_frame_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch);
int bsvd_yuv420_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc,
                          int32_t const_channels, float const_value, void *stream);
int bsvd_planar_to_yuv420(const float *src, void *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvDesc *desc,
                          void *stream);

/*
 * Frame I/O for any picture size: the four entry points above with a reflect pad on the way in and a crop on the way out, in the kernel.
 * The network needs H and W to be multiples of 4; the reference's callers pad the fp32 tensor on the right and bottom and crop the result
 * (denoising_model.py, padding_input / crop_output -- F.pad(x, (0, pw, 0, ph), mode='reflect') and y[..., :H, :W]).  These entry points
 * stand in for those two lines where the frames are uint8 or YUV 4:2:0 and never exist as fp32 on the host.  Added without a new
 * BSVD_ABI_VERSION: discover them by symbol (dlsym), like the YUV entry points.
 *
 * Picture size H x W: what the caller's frames / surfaces have.  Network size Hp x Wp: what the planar fp32 tensor has, Hp >= H, Wp >= W.
 *   in  (_pad):  dst [frames][C + const_channels][Hp][Wp]: element (r, c) = the converted picture element (refl_H(r), refl_W(c)),
 *                refl_N(i) = i for i < N, else 2 (N - 1) - i (the edge sample is not repeated: torch's 'reflect').  I.e. exactly
 *                "convert at picture size, then reflect-pad".  The constant channels are constant over the whole Hp x Wp plane.  With YUV
 *                the chroma upsampling clamps at the PICTURE's edges as in bsvd_yuv420_to_planar; the mirror acts on the RGB values.
 *   out (_crop): src [frames][C][Hp][Wp]: exactly "take src[..., :H, :W], then convert at picture size".  Pad rows and columns of src
 *                influence no sample; with YUV the chroma filter sees picture columns only.
 * Conversions, rounding and every other argument: as documented at the entry point of the same name without suffix.  The uint8 frames /
 * the surface are picture-sized (BsvdYuvDesc.row_pitch and frame_stride describe the picture-sized surface); no byte outside their
 * samples is read or written, and every destination element is written exactly once.  Hp == H and Wp == W is allowed (no pad).
 * All four return -3, naming the argument in bsvd_last_error(), for: a NULL pointer; frames, C, H or W <= 0; const_channels < 0; Hp < H or
 * Wp < W; a pad of a whole dimension or more (Hp - H >= H or Wp - W >= W: reflect is undefined there).  The YUV pair in addition for: H or
 * W odd; Hp odd; Wp not a multiple of 4 (the fp32 rows move as float4); and every desc / pitch / stride / alignment condition of
 * bsvd_yuv420_to_planar.  The uint8 pair takes any Hp, Wp and any alignment (float4 on the fp32 side when Wp % 4 == 0 and the tensor is
 * 16-byte aligned, scalars otherwise).
 * bsvd_yuv420_picture_bytes: as bsvd_yuv420_frame_bytes (row_pitch * H * 3 / 2), but H and W only need to be even.
 */
int bsvd_u8_to_planar_pad(const uint8_t *src, float *dst, int32_t frames, int32_t C, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                          int32_t src_hwc, int32_t const_channels, float const_val, void *stream);
int bsvd_planar_to_u8_crop(const float *src, uint8_t *dst, int32_t frames, int32_t C, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                           int32_t dst_hwc, int32_t reverse_channels, void *stream);
int64_t bsvd_yuv420_picture_bytes(int32_t H, int32_t W, int32_t pix_fmt, int32_t row_pitch);
int bsvd_yuv420_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                              const BsvdYuvDesc *desc, int32_t const_channels, float const_value, void *stream);
int bsvd_planar_to_yuv420_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                               const BsvdYuvDesc *desc, void *stream);

/*
 * YUV surfaces beyond NV12 / P010: the planar, 4:2:2 and 4:4:4 layouts software decoders, `ffmpeg -f rawvideo`, SDI capture cards, V4L2
 * devices and mastering pipelines hand over.  The entry points above and BsvdYuvDesc are unchanged; these take a BsvdYuvSurface instead.
 * Added without a new BSVD_ABI_VERSION: discover the five entry points by symbol (dlsym), like the YUV entry points above.
 *
 * A surface is described by its subsampling, its layout, its sample width and -- for 10 bit -- where the code sits in the 16-bit
 * little-endian word: high_bits = 1 is the P010 rule (code = word >> 6 in, word = code << 6 out; the low 6 bits ignored in, zero out),
 * high_bits = 0 the yuv4xxp10le rule (code = word & 1023 in; the high 6 bits ignored in, zero out).  Exactly ten combinations are served
 * (ffmpeg's names):
 *   yuv420p      4:2:0  PLANAR      8        |  yuv420p10le  4:2:0  PLANAR      10 low
 *   uyvy422      4:2:2  UYVY        8        |  yuyv422      4:2:2  YUYV        8
 *   nv16         4:2:2  SEMIPLANAR  8        |  p210le       4:2:2  SEMIPLANAR  10 high
 *   yuv422p      4:2:2  PLANAR      8        |  yuv422p10le  4:2:2  PLANAR      10 low
 *   yuv444p      4:4:4  PLANAR      8        |  yuv444p10le  4:4:4  PLANAR      10 low
 * every other one returns -3 naming the field that rules it out (4:2:0 SEMIPLANAR is NV12 / P010: bsvd_yuv420_*).
 * Layouts: PLANAR = three planes Y, Cb, Cr (chroma planes W/2 x H/2, W/2 x H, W x H samples for 4:2:0, 4:2:2, 4:4:4); SEMIPLANAR = a Y
 * plane and one plane of interleaved Cb Cr pairs; UYVY = one plane of Cb Y0 Cr Y1 groups; YUYV = one plane of Y0 Cb Y1 Cr groups.
 * Plane i has pitch[i] BYTES per row (0 = tight) and starts offset[i] bytes from the frame's first byte (offset[0] as given; 0 for planes 1
 * and 2 = directly behind the last row of the plane before, pitch included); frames are frame_stride bytes apart (0 = tight: the end of the
 * plane that ends last).  Planes must not share bytes.  pitch / offset of planes the layout does not have must be 0.
 *
 * Arithmetic: matrix, range, NOT-clamped decode, encode clamp, legal-code clamp and rounding (half to even) are word for word those of
 * bsvd_yuv420_to_planar / bsvd_planar_to_yuv420 -- a yuv420p surface gives the bits an NV12 surface of the same samples gives.  Chroma:
 *   4:2:0  as documented above.
 *   4:2:2  the horizontal half of it, nothing vertical: sample i is co-sited with luma column 2i.  In, LINEAR: even columns c[i], odd columns
 *          (c[i] + c[i+1]) / 2, clamped at the picture's right edge; NEAREST: both columns c[i].  Out, LINEAR: [1 2 1] / 4 over columns 2i-1,
 *          2i, 2i+1, edge-clamped; NEAREST: the mean of the two columns.
 *   4:4:4  no filter; `chroma` must still be a valid value and is ignored.
 * bsvd_yuv_to_planar / bsvd_planar_to_yuv: H and W multiples of 4; tensors as for the yuv420 pair.  bsvd_yuv_to_planar_pad /
 * bsvd_planar_to_yuv_crop: the rules of bsvd_yuv420_to_planar_pad / bsvd_planar_to_yuv420_crop (mirror after conversion, chroma filters
 * clamp at the picture's own edge, Wp a multiple of 4, pad below the dimension, Hp even with 4:2:0), for pictures of even H and W (4:2:0),
 * even W and any H >= 2 (4:2:2), any H, W >= 2 (4:4:4).  No byte outside a surface's samples is read or written -- pitch padding, the
 * bytes between planes and frames, and on input the ignored bits of a 10-bit word are all outside --, and every sample and every element
 * of the fp32 tensor is written exactly once.
 * All return -3, naming the argument in bsvd_last_error(), for: a NULL pointer; frames <= 0; a size the entry point does not take; an
 * unknown enum value; bits other than 8 / 10; a combination that is not served; a reserved field != 0; a pitch below the plane's row; a
 * negative offset; pitch / offset set for a plane the layout lacks; with 16-bit samples an odd pitch, offset, frame_stride or surface
 * pointer; frame_stride below one frame; a planar pointer that is not 16-byte aligned; const_channels < 0.  All of it without a device.
 * bsvd_yuv_frame_bytes: the bytes of one frame -- the end of the plane that ends last, tight or pitched -- for any picture size the
 * pad / crop pair takes; -1 on bad arguments.
 */
enum { BSVD_SUB_420 = 0, BSVD_SUB_422 = 1, BSVD_SUB_444 = 2 };
enum { BSVD_LAYOUT_PLANAR = 0, BSVD_LAYOUT_SEMIPLANAR = 1, BSVD_LAYOUT_UYVY = 2, BSVD_LAYOUT_YUYV = 3 };
typedef struct BsvdYuvSurface {
    int32_t subsampling, layout;
    int32_t bits;              /* 8 or 10 */
    int32_t high_bits;         /* 10 bit: 1 = code in the high bits of the word, 0 = in the low bits; 0 with 8 bit */
    int32_t matrix, full_range, chroma;   /* as in BsvdYuvDesc */
    int32_t reserved0;         /* must be 0 */
    int32_t pitch[3];          /* bytes per row of plane i; 0 = tight */
    int32_t reserved1;         /* must be 0 */
    int64_t offset[3];         /* bytes from the frame's first byte to plane i; 0 for planes 1, 2 = directly behind the plane before */
    int64_t frame_stride;      /* bytes; 0 = tight */
    int64_t reserved2;         /* must be 0 */
} BsvdYuvSurface;              /* 88 bytes */
int64_t bsvd_yuv_frame_bytes(int32_t H, int32_t W, const BsvdYuvSurface *surface);
int bsvd_yuv_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvSurface *surface,
                       int32_t const_channels, float const_value, void *stream);
int bsvd_planar_to_yuv(const float *src, void *dst, int32_t frames, int32_t H, int32_t W, const BsvdYuvSurface *surface,
                       void *stream);
int bsvd_yuv_to_planar_pad(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                           const BsvdYuvSurface *surface, int32_t const_channels, float const_value, void *stream);
int bsvd_planar_to_yuv_crop(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                            const BsvdYuvSurface *surface, void *stream);

/*
 * RGB surfaces: what callers hold who do not come through a video decoder -- OpenCV (bgr24), screen / window capture and GL / Vulkan
 * read-back (bgra, rgba, bgr0, pitched), 16-bit image sequences and mastering formats (rgb48le, gbrp10le .. gbrp16le, gbrap*), DRM / VAAPI
 * capture (x2rgb10le).  bsvd_u8_to_planar / bsvd_planar_to_u8 and their _pad / _crop forms are unchanged; these three take a BsvdRgbSurface.
 * Added without a new BSVD_ABI_VERSION: discover the three entry points by symbol (dlsym), like the YUV entry points above.
 *
 * A surface is a layout, a component count, a sample width and the place of each component:
 *   BSVD_RGB_PACKED        one plane of pixels; a pixel is `components` (3 or 4) samples, each one byte (bits = 8) or one little-endian
 *                          16-bit word with the code in the LOW `bits` bits (bits = 10, 12, 16; the high bits ignored in, zero out).
 *                          pos[c] = index of the sample of component c inside the pixel.
 *   BSVD_RGB_PACKED_X2_10  one plane of 32-bit little-endian words, three 10-bit fields and two unused top bits (ignored in, ones out):
 *                          field i is bits [10 i, 10 i + 10); pos[c] = the field of component c.  components = 3, bits = 10, fourth = 0.
 *                          x2rgb10le ((msb) 2 X | R | G | B (lsb)) is pos = {2, 1, 0}, x2bgr10le pos = {0, 1, 2}.
 *   BSVD_RGB_PLANAR        `components` (3 or 4) planes of W x H samples (one byte, or a 16-bit word as above); pos[c] = the plane of
 *                          component c.  ffmpeg's gbrp* is pos = {2, 0, 1}, gbrap* pos = {2, 0, 1, 3}.
 * Components: 0 = R, 1 = G, 2 = B, 3 = the fourth sample, which `fourth` names: 1 = alpha, 2 = a filler (rgb0, bgr0, 0rgb, 0bgr);
 * components = 3 goes with fourth = 0 and pos[3] = 0.  pos[0 .. components - 1] is a permutation of 0 .. components - 1.
 * Plane i has pitch[i] BYTES per row (0 = tight) and starts offset[i] bytes from the frame's first byte (offset[0] as given; 0 for a later
 * plane = directly behind the last row of the plane before, pitch included); frames are frame_stride bytes apart (0 = tight: the end of
 * the plane that ends last).  A plane occupies [offset, offset + pitch * H); planes must not share bytes.  pitch / offset of planes the
 * layout does not have must be 0.  With 16-bit samples pitch, offset, frame_stride and the surface pointer are multiples of 2, with
 * BSVD_RGB_PACKED_X2_10 of 4.
 *
 * Sizes: H x W is the picture (what the surface has), Hp x Wp the planar tensor.  Hp == H and Wp == W is the plain case; otherwise the
 * rules of bsvd_u8_to_planar_pad / bsvd_planar_to_u8_crop hold word for word: in, "convert at picture size, then reflect-pad" on the right
 * and bottom, the pad below the dimension; out, "take src[..., :H, :W], then convert".  Any Hp, Wp and any alignment (float4 on the fp32
 * side when Wp % 4 == 0 and the tensor is 16-byte aligned, scalars otherwise; the same bits either way).
 *
 * Arithmetic, in fp32, no contraction, with s = 2^(bits - 8), for each of R, G, B alike:
 *   in   full_range = 1:  v = (float)code / (float)(2^bits - 1)         (what bsvd_u8_to_planar does at 8 bits)
 *        full_range = 0:  v = ((float)code - 16 s) / (219 s)
 *        one subtraction (of 0 at full range) and one IEEE division.  NOT clamped: codes outside the legal range give v outside [0,1].
 *   out  c = rintf(fminf(fmaxf(v, 0), 1) * m + a), m = 2^bits - 1, a = 0 (full) or m = 219 s, a = 16 s (limited): one multiplication,
 *        one addition, round half to even; then clamped to [0, 2^bits - 1] or [16 s, 235 s].  At 8 bits full range: bsvd_planar_to_u8's.
 *   At full range every code of 8, 10, 12 and 16 bits comes back as itself; at limited range every legal code does and the others
 *   land on the nearest legal end.
 * dst of bsvd_rgb_to_planar is [frames][3 + const_channels][Hp][Wp], planes R, G, B, then the constant channels (constant over the whole
 * plane); src of bsvd_planar_to_rgb is [frames][3][Hp][Wp].
 * The fourth sample.  A filler is ignored on input and written as all ones on output (255, 2^bits - 1).  Alpha never meets the arithmetic:
 * with alpha_out != NULL the decode also writes the alpha codes, masked to `bits`, into a tight picture-sized side plane [frames][H][W]
 * of the container type (uint8_t or uint16_t), never padded; alpha_out == NULL ignores alpha.  The encode takes the alpha codes from
 * alpha_in (the same side plane, masked to `bits`), or writes the maximum code when alpha_in is NULL.
 * No byte outside a surface's samples is read or written -- pitch padding, the bytes between planes and frames, and on input the ignored
 * bits of a word are all outside --, and every sample, every element of the fp32 tensor and of alpha_out is written exactly once.
 * All return -3, naming the argument in bsvd_last_error(), without a device, for: a NULL src, dst or surface; frames <= 0; H or W <= 0;
 * Hp < H or Wp < W; a pad of a whole dimension or more; an unknown layout; components other than 3 / 4; bits other than 8 / 10 / 12 / 16
 * or not served by the layout; fourth outside 0 .. 2 or at odds with components; full_range other than 0 / 1; pos not a permutation;
 * a reserved field != 0; a pitch below the plane's row; a negative offset; pitch / offset set for a plane the layout lacks; planes
 * sharing bytes; frame_stride below one frame; a pitch, offset, frame_stride or surface / alpha pointer off the sample's alignment; a
 * planar pointer that is not 4-byte aligned; alpha_out / alpha_in given for a surface without alpha; const_channels < 0.
 * bsvd_rgb_frame_bytes: the bytes of one frame, tight or pitched; -1 on bad arguments.
 */
enum { BSVD_RGB_PACKED = 0, BSVD_RGB_PACKED_X2_10 = 1, BSVD_RGB_PLANAR = 2 };
enum { BSVD_RGB_FOURTH_NONE = 0, BSVD_RGB_FOURTH_ALPHA = 1, BSVD_RGB_FOURTH_FILLER = 2 };
typedef struct BsvdRgbSurface {
    int32_t layout;
    int32_t components;        /* 3 or 4: samples per pixel (PACKED) / planes (PLANAR); 3 with PACKED_X2_10 */
    int32_t bits;              /* 8 | 10 | 12 | 16; 10 with PACKED_X2_10 */
    int32_t pos[4];            /* where R, G, B and the fourth sample sit */
    int32_t fourth;            /* BSVD_RGB_FOURTH_* */
    int32_t full_range;        /* 1 = codes span [0, 2^bits - 1], 0 = [16 s, 235 s] */
    int32_t pitch[4];          /* bytes per row of plane i; 0 = tight */
    int32_t reserved0;         /* must be 0 */
    int64_t offset[4];         /* bytes from the frame's first byte to plane i; 0 for planes 1 .. 3 = directly behind the plane before */
    int64_t frame_stride;      /* bytes; 0 = tight */
    int64_t reserved;          /* must be 0 */
} BsvdRgbSurface;              /* 104 bytes */
int64_t bsvd_rgb_frame_bytes(int32_t H, int32_t W, const BsvdRgbSurface *surface);
int bsvd_rgb_to_planar(const void *src, float *dst, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                       const BsvdRgbSurface *surface, void *alpha_out, int32_t const_channels, float const_value, void *stream);
int bsvd_planar_to_rgb(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                       const BsvdRgbSurface *surface, const void *alpha_in, void *stream);

/*
 * The output finish: what happens between the network's [frames][3][Hp][Wp] fp32 result and the surface, on the device -- a denoise
 * strength (bsvd_blend_planar) and dither at the quantiser (the `_d` forms of the three surface encoders).  Added without a new
 * BSVD_ABI_VERSION: discover the four entry points by symbol (dlsym), like the YUV and RGB entry points above.  Every existing entry point
 * is unchanged, signature and bits; the bsvd_planar_to_u8* kernels have no dithered form (rgb24 is a BsvdRgbSurface, with the same bits).
 *
 * bsvd_blend_planar mixes the network's output y (planes R, G, B, frames y_frame_stride ELEMENTS apart) with the input x the frames came
 * from (its first three planes; x_frame_stride differs because x carries the noise-map plane), in place on y, over the whole Hp x Wp plane
 * (the pad region of x holds mirror images of the picture: harmless).  s_luma / s_chroma in [0, 1]: 1 = the network's result, 0 = the
 * source; luma_w = the Kr, Kg, Kb of the stream's matrix.  Arithmetic in fp32, no contraction, per pixel and component c:
 *     m_c   = s_chroma * y_c + om * x_c                     two products, one sum; om = (float)(1 - s_chroma), computed once on the host
 *     l     = fmaf(w_B, x_B - y_B, fmaf(w_G, x_G - y_G, w_R * (x_R - y_R)))
 *     out_c = m_c + (s_chroma - s_luma) * l                 the factor is one fp32 subtraction on the host
 * The ends are exact for finite values: s_luma = s_chroma = 1 gives y bit for bit, s_luma = s_chroma = 0 gives x bit for bit, and with
 * s_luma == s_chroma the luma term is an exact zero (out_c = m_c).  (A value that is -0 comes out +0.)  One float4 per plane row per lane
 * when Wp % 4 == 0, both pointers are 16-byte aligned and both strides multiples of 4; scalars otherwise; the same bits either way.
 * Returns -3, naming the argument in bsvd_last_error(), without a device, for: a NULL y, x or luma_w; frames, Hp or Wp <= 0; a frame
 * stride below 3 planes; a strength (or a luma weight) outside [0, 1] or not finite; a pointer that is not 4-byte aligned.
 *
 * Dither.  bsvd_planar_to_yuv420_crop_d, bsvd_planar_to_yuv_crop_d and bsvd_planar_to_rgb_d take the arguments of the functions they are
 * named after plus a BsvdDither (Hp == H, Wp == W is the plain case); with mode = BSVD_DITHER_NONE they give those functions' bytes.
 * A value d, in units of one code, joins the scaled, not yet rounded value t right before the encoder's own clamp and rintf, whose order
 * stays what it is: YUV rint(clamp(t + d, lo, hi)), RGB clamp(rint(t + d), lo, hi).  t + d is one fp32 addition.  d lies in the OPEN
 * interval (-0.5, 0.5) in both modes and is rectangular, not triangular: a value that is a whole code already is never moved (at every
 * served bit depth), and round-half-to-even meets no tie it did not have before.  Alpha and filler samples are never dithered.
 * A sample is named by its component (0, 1, 2: Y, Cb, Cr / R, G, B), the row and column of its OWN grid (the picture's for luma, 4:4:4 and
 * RGB; the chroma grid for subsampled chroma) and its frame:
 *   BSVD_DITHER_ORDERED  d = (B[(row + r_c) & 7][(col + q_c) & 7] + 0.5) / 64 - 0.5, B the 8 x 8 Bayer matrix (0 .. 63, B[0][0..7] =
 *                        0 32 8 40 2 34 10 42), (r_c, q_c) = (0, 0), (2, 5), (5, 2) for components 0, 1, 2.  Static over frames.
 *   BSVD_DITHER_RANDOM   d = ((h >> 8) + 0.5) 2^-24 - 0.5, evaluated as ((float)((int)(h >> 8) - 2^23) + 0.5f) * 2^-24 (every step exact in
 *                        fp32) and limited to +-(0.5 - 2^-7), ORDERED's largest |d|: two spacings of fp32 at the highest 16-bit codes below the
 *                        tie, so that the ROUNDED sum t + d of a whole code (or of one a round trip left one spacing off) never reaches it.  h = fmix32(kf ^ p), fmix32 = MurmurHash3's 32-bit finaliser (h ^= h >> 16;
 *                        h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16); with n = (uint64)(frame0 + f) * 4 + component,
 *                        kf = fmix32(seed ^ fmix32((uint32)n ^ fmix32((uint32)(n >> 32)))); p = (uint32)col + (uint32)row * 0x9e3779b1.
 *                        frame0 + f is the frame's STREAM index: a clip encoded in one call of T frames and in T calls of one frame with
 *                        frame0 counted up gives the same bytes.
 * The `_d` functions return -3 for what the functions they are named after refuse, and for: a NULL dither; a mode outside 0 .. 2; a
 * negative frame0; reserved != 0.
 */
enum { BSVD_DITHER_NONE = 0, BSVD_DITHER_ORDERED = 1, BSVD_DITHER_RANDOM = 2 };
typedef struct BsvdDither {
    int32_t mode;              /* BSVD_DITHER_* */
    uint32_t seed;             /* RANDOM: the stream's seed */
    int64_t frame0;            /* RANDOM: the stream index of the call's first frame */
    int64_t reserved;          /* must be 0 */
} BsvdDither;                  /* 24 bytes */
int bsvd_blend_planar(float *y, int64_t y_frame_stride, const float *x, int64_t x_frame_stride, int32_t frames, int32_t Hp, int32_t Wp,
                      float s_luma, float s_chroma, const float luma_w[3], void *stream);
int bsvd_planar_to_yuv420_crop_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                                 const BsvdYuvDesc *desc, const BsvdDither *dither, void *stream);
int bsvd_planar_to_yuv_crop_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                              const BsvdYuvSurface *surface, const BsvdDither *dither, void *stream);
int bsvd_planar_to_rgb_d(const float *src, void *dst, int32_t frames, int32_t Hp, int32_t Wp, int32_t H, int32_t W,
                         const BsvdRgbSurface *surface, const void *alpha_in, const BsvdDither *dither, void *stream);

/*
 * The noise level of a frame, estimated on the device.  bsvd_c64 is non-blind: its fourth input channel is the noise map, which the
 * reference fills with a constant the caller knows (temp_denoise's sigma map, validation_seq_infer.py:19-21).  A camera, SDI or ffmpeg
 * feed comes without one.  These entry points stand in for that constant: bsvd_estimate_sigma computes one sigma per frame from the planar
 * fp32 tensor the *_to_planar entry points build, bsvd_fill_sigma_plane writes per-frame values from DEVICE memory into the noise-map
 * plane -- nothing crosses to the host and nothing on the stream waits for it.  Added without a new BSVD_ABI_VERSION: discover the three
 * entry points by symbol (dlsym), like the YUV entry points above.
 *
 * The estimate, exactly (tests/sigma_model.py reproduces histogram and sigma bit for bit):
 *   input     x [frames][.][Hp][Wp] fp32, frames `frame_stride` FLOATS apart (>= channels * Hp * Wp), rows Wp apart.  The picture is the
 *             top-left H x W of each plane (3 <= H <= Hp, 3 <= W <= Wp): the mirror images of a padded tensor are not sampled.
 *   samples   the interior pixels 1 <= r <= H - 2, 1 <= c <= W - 2 of the first `channels` planes, pooled per frame.
 *   response  the Laplacian-difference mask [1 -2 1; -2 4 -2; 1 -2 1] in fp32, in this order:
 *             r = (4 x_c - 2 ((x_n + x_s) + (x_w + x_e))) + ((x_nw + x_ne) + (x_sw + x_se)).  Every coefficient is a power of two.
 *   bin       q = min(floor(|r| * 4096), 4095) into one histogram of 4096 uint32 counts per frame; a sample whose r is not finite is
 *             not counted.  Integer adds only: the histogram does not depend on the launch shape.
 *   finish    N = sum of the counts, k = the first bin with 2 cum[k] >= N, before = cum[k] - h[k]; in double,
 *             med = k + (N - 2 before) / (2 h[k]); sigma = med * K with K = 1 / (4096 * 6 * 0.6744897501960817) (6: the mask's L2 norm;
 *             0.6745: the median of |N(0,1)|), then * gain, clamped to [lo, hi], converted to fp32.  N == 0 gives lo.
 * The median of |r| saturates where half the samples reach the last bin: estimates stop at 1 / (6 * 0.6745) = 0.2471 (63 / 255).
 * What is known about it: on synthetic frames with white Gaussian noise it is within 0.7 / 255 of the truth for sigma 2 .. 30 / 255 on
 * frames of 64 x 96 and larger (profiles/sigma_auto.txt).  Nothing has been measured on real footage.  A source with subsampled chroma gives correlated,
 * chroma-smoothed RGB noise and the estimate reads LOW there: that is what `gain` is for.
 *
 * bsvd_sigma_workspace_bytes(frames): the bytes of `workspace`, frames * 4096 * 4; -1 for frames <= 0.
 * bsvd_estimate_sigma: zeroes the workspace itself, on the stream; afterwards the workspace holds the [frames][4096] uint32 histograms and
 *   sigma_out[frames] the estimates (fp32, device memory).  Rows move as float4 when x is 16-byte aligned and Wp and frame_stride are
 *   multiples of 4, as scalars otherwise.  Returns -3, naming the argument in bsvd_last_error(), for: a NULL pointer; a pointer that is not
 *   4-byte aligned; frames outside 1 .. 65535; channels <= 0; H or W below 3; Hp < H or Wp < W; frame_stride below channels * Hp * Wp;
 *   channels * (H - 2) * (W - 2) >= 2^32; gain not positive and finite; lo or hi not finite, lo < 0 or lo > hi.  All of it without a device.
 * bsvd_fill_sigma_plane: x [frames][>= channels + 1][Hp][Wp]; every element of plane `channels` of frame t becomes sigma_dev[t].  float4
 *   stores when x is 16-byte aligned and Hp * Wp and frame_stride are multiples of 4.  -3 for: a NULL or misaligned pointer; frames outside
 *   1 .. 65535; channels, Hp or Wp <= 0; frame_stride below (channels + 1) * Hp * Wp.
 */
int64_t bsvd_sigma_workspace_bytes(int32_t frames);
int bsvd_estimate_sigma(const float *x, int32_t frames, int32_t channels, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride,
                        float gain, float lo, float hi, void *workspace, float *sigma_out, void *stream);
int bsvd_fill_sigma_plane(float *x, int32_t frames, int32_t channels, int32_t Hp, int32_t Wp, int64_t frame_stride, const float *sigma_dev,
                          void *stream);

/*
 * The noise-level function (NLF) of a frame and the per-pixel noise map made from it.  One sigma per frame fits white Gaussian noise; the
 * noise of a camera or a decoder depends on the signal level (shot noise through a tone curve), and the network reads its noise-map plane
 * per pixel.  bsvd_estimate_nlf computes sigma as a function of local intensity, sixteen values per frame; bsvd_fill_nlf_plane writes the
 * map from them.  Both run on the device from the planar fp32 tensor the *_to_planar entry points build; nothing crosses to the host.
 * Added without a new BSVD_ABI_VERSION: discover the entry points by symbol (dlsym), like the sigma entry points above.
 *
 * Exactly (tests/nlf_model.py reproduces histogram, curve and map bit for bit), with NLF_LEVELS = 16 and NLF_BINS = 1024:
 *   input     x [frames][>= 3][Hp][Wp] fp32, frames `frame_stride` FLOATS apart, rows Wp apart.  The picture is the top-left H x W of each
 *             plane (3 <= H <= Hp, 3 <= W <= Wp).
 *   samples   the interior pixels 1 <= r <= H - 2, 1 <= c <= W - 2 of the first three planes, pooled per frame.
 *   response  r: the Laplacian-difference mask of bsvd_estimate_sigma, in its order of operations.
 *   box sum   S of the same nine values, in fp32, in this order: row = (x_w + x_c) + x_e for each of the three rows,
 *             S = (row_n + row_c) + row_s.  The box is orthogonal to the mask (1 - 2 + 1 = 0): under white noise S is uncorrelated with
 *             r, so binning by it does not bias the median.
 *   level     l = clamp(floor(S * c169), 0, 15) with c169 = 16 / 9 rounded to fp32 once; +inf gives 15, anything not >= 0 gives 0.
 *   bin       q = min(floor(|r| * 1024), 1023); a sample is counted iff r is finite.  Counts are uint32 [frames][16][1024].  Integer adds
 *             only: the histogram does not depend on the launch shape.
 *   curve     c[t][l], fp32.  A level with at least min_count samples is VALID: N = its counts, k = the first bin with 2 cum[k] >= N,
 *             before = cum[k] - h[k]; in double med = k + (N - 2 before) / (2 h[k]), value = med * K with
 *             K = 1 / (1024 * 6 * 0.6744897501960817), then * gain, clamped to [lo, hi], converted to fp32.  A level that is not valid
 *             takes the value of the nearest valid level, the lower one on a tie.  No valid level: every level gets the pooled value, the
 *             same finish on the histogram summed over the levels (N == 0 gives lo).  No smoothing across levels, no temporal filter.
 *   map       for every pixel of the whole Hp x Wp plane: the box sums S_R, S_G, S_B of planes 0, 1, 2 with row and column indices clamped
 *             to the plane (replicate); u = ((S_R + S_B) + 2 S_G) * c1636 - 0.5 with c1636 = 16 / 36 rounded to fp32 once, multiply and
 *             subtract rounded separately; u clamped to [0, 15], not-a-number gives 0; i = min((int)u, 14), f = u - i;
 *             map = c[i] + f * (c[i + 1] - c[i]) in fp32, the product rounded before the add.  Level l's value sits at its centre.
 * Two consequences: a flat curve gives exactly that value at every pixel (f * 0 = 0: the bits bsvd_fill_sigma_plane writes), and the map is
 * finite whatever the colour planes hold (c is finite, 0 <= f <= 1).
 * What is known about it: profiles/noise_curve.txt, on synthetic signal-dependent noise only.  Nothing has been measured on real footage,
 * and a per-pixel map is outside what the reference's checkpoints were trained on (a constant plane): bsvd_vst_* below turn the same curve
 * into a variance-stabilising transform, which keeps the constant plane.
 *
 * bsvd_nlf_workspace_bytes(frames): the bytes of `workspace`, frames * 16 * 1024 * 4; -1 for frames <= 0.
 * bsvd_estimate_nlf: zeroes the workspace itself, on the stream; afterwards the workspace holds the [frames][16][1024] uint32 histograms
 *   and curve_out[frames][16] the curves (fp32, device memory).  Rows move as float4 when x is 16-byte aligned and Wp and frame_stride are
 *   multiples of 4, as scalars otherwise.  Returns -3, naming the argument in bsvd_last_error(), for: a NULL pointer; a pointer that is not
 *   4-byte aligned; frames outside 1 .. 65535; H or W below 3; Hp < H or Wp < W; frame_stride below 3 * Hp * Wp;
 *   3 * (H - 2) * (W - 2) >= 2^32; gain not positive and finite; lo or hi not finite, lo < 0 or lo > hi; min_count < 1.  All of it without
 *   a device.
 * bsvd_finish_nlf: the curve step alone, from [frames][16][1024] uint32 histograms the caller holds in device memory (a caller who pools
 *   histograms over frames, or a test of the curve rules).  The workspace is only read.  -3 as above for its arguments.
 * bsvd_fill_nlf_plane: x [frames][>= channels + 1][Hp][Wp], channels >= 3; every element of plane `channels` of frame t is written from
 *   planes 0 .. 2 of that frame and curve_dev[t][0 .. 15] (device memory).  float4 loads and stores when x is 16-byte aligned and Wp and
 *   frame_stride are multiples of 4.  -3 for: a NULL or misaligned pointer; frames outside 1 .. 65535; channels < 3; Hp or Wp <= 0;
 *   frame_stride below (channels + 1) * Hp * Wp.
 */
int64_t bsvd_nlf_workspace_bytes(int32_t frames);
int bsvd_estimate_nlf(const float *x, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride,
                      float gain, float lo, float hi, int32_t min_count, void *workspace, float *curve_out /*[frames][16]*/, void *stream);
int bsvd_finish_nlf(const void *workspace, int32_t frames, float gain, float lo, float hi, int32_t min_count, float *curve_out, void *stream);
int bsvd_fill_nlf_plane(float *x, int32_t frames, int32_t channels, int32_t Hp, int32_t Wp, int64_t frame_stride,
                        const float *curve_dev /*[frames][16]*/, void *stream);

/*
 * The variance-stabilising transform (VST) of a noise-level curve.  The per-pixel map above is outside what the reference's checkpoints
 * were trained on; the transform is the remedy that stays inside it: intensities are remapped by g(I) ~ integral dI / sigma(I), so that
 * the noise has ONE standard deviation sigma' at every level, the network runs with a constant noise plane at sigma', and the result is
 * mapped back with the inverse of g.  bsvd_vst_build makes the tables of g from curves in device memory, bsvd_vst_forward and
 * bsvd_vst_inverse apply them in place.  Added without a new BSVD_ABI_VERSION: discover the three entry points by symbol (dlsym), like the
 * NLF entry points above.
 *
 * Exactly (tests/vst_model.py reproduces tables, forward and inverse bit for bit), with N = 1024 intervals over [0, 1]:
 *   table set 2052 floats: G[0 .. N] at 0, sigma' at 1025, zeros at 1026 and 1027, R[0 .. N - 1] at 1028.
 *   s_j       j = 0 .. N - 1, the curve c[0 .. 15] at the midpoint of interval j: u = (j + 0.5) * (16 / N) - 0.5 (exact in fp32), clamped to
 *             [0, 15]; i = min((int)u, 14); f = u - i; s = c[i] + f * (c[i + 1] - c[i]) in fp32, the product rounded before the add
 *             (bsvd_fill_nlf_plane's rule); then s = s >= floor ? s : floor (not-a-number gives floor) and s = s <= 1 ? s : 1.
 *   build     in double, ascending j, every operation rounded once: w_j = 1.0 / (double)s_j; F_0 = 0; F_{j+1} = F_j + w_j;
 *             G[j] = (float)(F_j / F_N) for j = 0 .. N (G[0] = 0 and G[N] = 1 exactly);
 *             R[j] = (float)(1.0 / ((double)G[j + 1] - (double)G[j])); sigma' = (float)(N / F_N), the harmonic mean of the clamped curve.
 *   forward   t = x * 1024; k = t >= 1023 ? 1023 : (t >= 0 ? (int)t : 0) (not-a-number gives 0); fr = t - (float)k;
 *             y = G[k] + fr * (G[k + 1] - G[k]) in fp32, the difference, the product and the add rounded separately.  Values outside [0, 1]
 *             continue on the end interval's line (limited-range YUV produces them).  No clamp to G[k + 1] is applied: the model finds the
 *             forward non-decreasing over every 16-bit code and over every knot +- 1 ulp for the curves of tests/test_vst_cpu.py.
 *   inverse   k = the largest index in 0 .. 1023 with G[k] <= y, 0 if there is none (not-a-number gives 0);
 *             x = ((float)k + (y - G[k]) * R[k]) * (1 / 1024) in fp32, each operation rounded separately (the last is exact).
 * floor is refused below 2^-10 and above 1: consecutive G then differ by at least floor / 1024 >= 16 ulp, so G is strictly increasing and R
 * is finite.  The build is in double so that the tables do not depend on a device fp32 division; the per-pixel paths multiply only.
 * Not-a-number in gives not-a-number out; +-inf and -0.0 follow the formulas; no index ever leaves the table.
 * What is known about it: profiles/vst.txt, on synthetic signal-dependent noise only.  No trained checkpoint has been run through it, so
 * its effect on denoising quality has not been measured, and nothing has been measured on real footage.  The inverse is the algebraic one:
 * a nonlinear inverse of a denoised mean is biased where the curve bends sharply relative to sigma', and no unbiased-inverse correction is
 * applied.  The transform changes the tone curve the network sees.
 *
 * bsvd_vst_build: curves [n][16] (device memory) -> tables [n][2052] (device memory), on the stream, nothing crosses to the host.  One
 *   workgroup per curve; the 1024 adds of F are one lane's, in order.  Returns -3, naming the argument in bsvd_last_error(), without a
 *   device, for: a NULL or misaligned pointer; n outside 1 .. 65535; floor outside [2^-10, 1] or not finite.
 * bsvd_vst_forward: in place on planes 0 .. 2 of x [frames][>= 3][Hp][Wp], frames `frame_stride` FLOATS apart.  Frame t uses the table set
 *   at tables + t * table_stride * 2052; table_stride == 0: one set for all frames.  fill_plane >= 3: every element of that plane of frame
 *   t becomes that frame's sigma' (the noise-map plane); fill_plane < 0: no plane is written (a blind model has none).  Planes move as
 *   float4 when x is 16-byte aligned and Hp * Wp and frame_stride are multiples of 4, as scalars otherwise; the same bits either way.  -3
 *   for: a NULL or misaligned pointer; frames outside 1 .. 65535; Hp or Wp <= 0; fill_plane in 0 .. 2; frame_stride below the planes it
 *   spans (3, or fill_plane + 1); table_stride outside 0 .. 65535.
 * bsvd_vst_inverse: in place on the three planes of y, frames y_frame_stride ELEMENTS apart (like bsvd_blend_planar), the same table
 *   addressing and the same float4 rule.  -3 as for bsvd_vst_forward.
 */
int bsvd_vst_build(const float *curves /*[n][16]*/, int32_t n, float floor, float *tables /*[n][2052]*/, void *stream);
int bsvd_vst_forward(float *x, int32_t frames, int32_t Hp, int32_t Wp, int64_t frame_stride, int32_t fill_plane, const float *tables,
                     int64_t table_stride, void *stream);
int bsvd_vst_inverse(float *y, int64_t y_frame_stride, int32_t frames, int32_t Hp, int32_t Wp, const float *tables, int64_t table_stride,
                     void *stream);

/*
 * Film grain: the statistics of the noise the network removed, and clean synthetic grain from a model fitted to them.  The denoise
 * strength (bsvd_blend_planar) mixes the removed signal itself back -- chroma blotches, fixed-pattern residue and compression artefacts
 * with it.  A grain MODEL keeps only two things of the removed noise: its standard deviation against the result's brightness and its
 * spatial autocorrelation ("grain size").  bsvd_grain_stats reduces a source / result pair to 256 integers per frame; the fit is the
 * host's (bsvd_amd/frame_io.py, GrainModel: 3 x 16 standard deviations, 3 x 24 coefficients of a causal lag-3 autoregression, a
 * 128 x 128 unit-variance template per component); bsvd_grain_apply adds grain from the templates to the result, in place.  Added
 * without a new BSVD_ABI_VERSION: discover the three entry points by symbol (dlsym), like the VST entry points above.
 *
 * The statistics, exactly (tests/grain_model.py reproduces all 256 integers bit for bit):
 *   input     x (the source) and y (the result) [frames][>= 3][Hp][Wp] fp32, planes R, G, B, frames x_frame_stride / y_frame_stride FLOATS
 *             apart, rows Wp apart.  The picture is the top-left H x W of each plane (4 <= H <= Hp, 13 <= W <= Wp); nothing outside it is
 *             read (the mirror images of a padded tensor would count twice).
 *   pixel     in fp32, every operation rounded once: d_c = x_c - y_c;
 *             n0 = fmaf(w_B, d_B, fmaf(w_G, d_G, w_R * d_R)) (bsvd_blend_planar's luma term, in its order); n1 = d_B - n0; n2 = d_R - n0;
 *             ly = fmaf(w_B, y_B, fmaf(w_G, y_G, w_R * y_R)); t = ly * 16; level l = t >= 15 ? 15 : (t >= 0 ? (int)t : 0) (NaN gives 0);
 *             q_k = (int)rintf(min(max(n_k * 4096, -2047), 2047)), halves to even.
 *             A pixel with a non-finite n_k is NOT COUNTED, and all three of its q are 0.
 *   moments   over the counted pixels of the picture, per level l: N[l], and for k = 0 .. 2 the sums of q_k and of q_k^2.
 *   products  for k = 0 .. 2 and the 46 lags (dy, dx) -- dy = 0 with dx = 0 .. 6, then dy = 1, 2, 3 with dx = -6 .. 6 each, in that order --
 *             A[k][lag] = the sum over the anchors p = (r, c), 0 <= r <= H - 4 and 6 <= c <= W - 7, of q_k(p) q_k(p + (dy, dx)).  The
 *             anchor set is the same for every lag: (H - 3) (W - 12) anchors.  These are the lags whose differences a causal lag-3
 *             neighbourhood of 24 taps meets in its Yule-Walker system.
 *   layout    per frame 256 int64: N[16] at 0, sum q_k at 16 + 16 k + l, sum q_k^2 at 64 + 16 k + l, A[k][lag] at 112 + 46 k + lag,
 *             zeros at 250 .. 255.
 * Every accumulated quantity is an integer: the result does not depend on the launch shape.  Sums are exact in int64 for every frame
 * the other checks admit (|q| <= 2047: a product is below 2^22).
 *
 * The synthesis, exactly (tests/grain_model.py reproduces it bit for bit), per pixel (r, c) of the whole Hp x Wp plane of frame t:
 *   block     (by, bx) = (r >> 5, c >> 5); n = (uint64)(frame0 + t) * 4 + 3 (the dither's frame number with the component no dither
 *             uses); kf = fmix32(seed ^ fmix32((uint32)n ^ fmix32((uint32)(n >> 32)))); h = fmix32(kf ^ ((uint32)bx + (uint32)by *
 *             0x9e3779b1)) with fmix32 as in BsvdDither above; oy = ((h >> 16) * 97) >> 16, ox = ((h & 0xffff) * 97) >> 16: both 0 .. 96.
 *   sample    g_k = templates[k][oy + (r & 31)][ox + (c & 31)].  Neighbouring blocks are cut from unrelated places: no overlap blending.
 *   scale     ly as above; u = ly * 16 - 0.5 (two roundings), clamped to [0, 15], NaN gives 0; i = min((int)u, 14); f = u - i;
 *             s_k = std[k][i] + f * (std[k][i + 1] - std[k][i]), the product rounded before the add (bsvd_fill_nlf_plane's rule).
 *   noise     n_k = (amount * s_k) * g_k.
 *   to RGB    d_R = n2 + n0; d_B = n1 + n0; d_G = (n0 - (w_R * d_R + w_B * d_B)) * inv_wg, two products, one sum, one difference, one
 *             product; y_c = y_c + d_c.  All fp32, no contraction.  inv_wg is the caller's 1 / w_G.
 * What is known about it: profiles/film_grain.txt, on synthetic grain only.  Nothing has been measured on real footage, and no encoder
 * has read the model: there is no AV1 / filmgrn1 table writer.  No overlap blending of blocks; no temporal pooling of the statistics.
 *
 * bsvd_grain_stats_bytes(frames): the bytes of `workspace`, frames * 256 * 8; -1 for frames <= 0.
 * bsvd_grain_stats: zeroes the workspace itself, on the stream; afterwards it holds [frames][256] int64.  Returns -3, naming the argument
 *   in bsvd_last_error(), without a device, for: a NULL pointer; x or y not 4-byte aligned, workspace not 8-byte aligned; frames outside
 *   1 .. 65535; H < 4 or W < 13; Hp < H or Wp < W; a frame stride below 3 * Hp * Wp; a weight that is not finite.
 * bsvd_grain_apply: y [frames][3][Hp][Wp], frames y_frame_stride FLOATS apart, in place.  templates: [3][128][128] fp32 in DEVICE memory;
 *   std: [3][16] fp32 in HOST memory (read during the call).  Rows move as float4 when y is 16-byte aligned and Wp and the stride are
 *   multiples of 4, as scalars otherwise; the same bits either way.  amount == 0 or an all-zero std: 0 is returned and nothing is
 *   launched.  -3 for: a NULL pointer; y or templates not 4-byte aligned; frames outside 1 .. 65535; Hp or Wp <= 0; a stride below
 *   3 * Hp * Wp; amount, a std value, a weight or inv_wg not finite; amount or a std value negative; frame0 negative.
 */
int64_t bsvd_grain_stats_bytes(int32_t frames);
int bsvd_grain_stats(const float *x, int64_t x_frame_stride, const float *y, int64_t y_frame_stride, int32_t frames, int32_t H, int32_t W,
                     int32_t Hp, int32_t Wp, const float luma_w[3], void *workspace /*[frames][256] int64*/, void *stream);
int bsvd_grain_apply(float *y, int64_t y_frame_stride, int32_t frames, int32_t Hp, int32_t Wp, const float *templates /*[3][128][128], device*/,
                     const float *std /*[3][16], host*/, float amount, const float luma_w[3], float inv_wg, uint32_t seed, int64_t frame0,
                     void *stream);

/*
 * What a scene-cut detector needs from a frame, computed on the device.  Each temporal-fusion conv mixes a frame with its two neighbours; a
 * caller who knows where a scene starts passes halo_prev = NULL / halo_next = NULL there (a clip end in mid-stream).  These two entry points
 * serve the caller who does not know: they reduce the planar fp32 tensor the *_to_planar entry points build -- so the result does not depend
 * on the pixel format -- to one integer per frame pair; the decision (a threshold on it) is the host's.  Added without a new
 * BSVD_ABI_VERSION: discover the two entry points by symbol (dlsym), like the sigma entry points above.
 *
 * Exactly (tests/scene_model.py reproduces both results bit for bit):
 *   input   x [frames][>= 3][Hp][Wp] fp32, frames `frame_stride` FLOATS apart (>= 3 * Hp * Wp), rows Wp apart.  The picture is the top-left
 *           H x W of each plane (0 <= H <= Hp, 0 <= W <= Wp); only its full 16 x 16 blocks count: GH = H / 16, GW = W / 16.
 *   value   q = clamp(rint(255 v), 0, 255) per plane value, halves to even, NaN -> 0; L = qR + 2 qG + qB per pixel (0 .. 1020).
 *   grid    grid[t][by][bx] (int32, [frames][GH * GW]) = the sum of L over block (by, bx): 0 .. 261120.  (256 pixels a block: white noise
 *           is averaged down by 16.)
 *   sad     sad[t] (uint64) = sum over the blocks of |grid[t][b] - grid[t-1][b]|; for t = 0, prev_grid [GH * GW] stands in for grid[-1],
 *           and prev_grid == NULL gives sad[0] = 0.
 * Integer sums only: neither result depends on the launch shape.
 *
 * bsvd_scene_grid: rows move as float4 when x is 16-byte aligned and Wp and frame_stride are multiples of 4, as scalars otherwise.
 *   GH * GW == 0 is valid: nothing is written and nothing launched (grid may be NULL then).  Returns -3, naming the argument in
 *   bsvd_last_error(), for: a NULL or misaligned pointer; frames outside 1 .. 65535; H or W negative; Hp or Wp not positive; Hp < H or
 *   Wp < W; frame_stride below 3 * Hp * Wp.  All of it without a device.
 * bsvd_scene_diff: zeroes sad[frames] itself, on the stream.  blocks = GH * GW; blocks == 0 is valid and leaves every sum 0 without a
 *   kernel.  -3 for: frames outside 1 .. 65535; blocks negative; sad NULL or not 8-byte aligned; grid NULL with blocks > 0; grid or
 *   prev_grid not 4-byte aligned.
 */
int bsvd_scene_grid(const float *x, int32_t frames, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int64_t frame_stride, int32_t *grid,
                    void *stream);
int bsvd_scene_diff(const int32_t *grid, const int32_t *prev_grid, int32_t frames, int32_t blocks, uint64_t *sad, void *stream);

/*
 * Frame-window sharding: gathers the channel slice [c0, c0+n) of one NHWC frame into
 * a compact [H*W][n] buffer -- the message a rank sends to its temporal neighbour
 * (first frame, c0 = 0 -> the left neighbour's halo_next; last frame, c0 = fold -> the right
 * neighbour's halo_prev).  dtype BSVD_F32: a plain float range (also right for WHOLE 16-channel chunks of a split16 frame);
 * dtype BSVD_F16X3: one 8-channel half chunk of a split16 frame (n == 8, c0 % 8 == 0; the fold-8 layers of the c32-sized
 * networks) -> dst [H*W][hi x8 | lo x8], which bsvd_conv3x3 reads as a compact halo (pstride = 8, coff = 0).
 */
int bsvd_halo_pack(const void *frame, void *dst, int32_t HW, int32_t C, int32_t c0, int32_t n,
                   int32_t dtype, void *stream);

/*
 * Inverse of bsvd_halo_pack: scatters a compact [H*W][n] slice into channels [c0, c0+n) of an NHWC frame, for hosts that
 * keep a materialised neighbour frame (the reference's own `left_fold_2fold` / `center` buffers, bsvd_arch.py:112-113)
 * instead of handing the slice to bsvd_conv3x3 as halo_prev / halo_next (which reads compact slices in place:
 * pstride = n, coff = 0).  The other channels of `frame` are left untouched.
 */
int bsvd_halo_unpack(const void *src, void *frame, int32_t HW, int32_t C, int32_t c0, int32_t n,
                     int32_t dtype, void *stream);

/*
 * Scratch bytes bsvd_conv3x3(args) needs beyond the caller's tensors.  0 for every configuration of this ABI version
 * (all staging is LDS / registers; the library never allocates) -- exported so a host that sizes its arena from the
 * library keeps working if a later version wants a workspace.  Validates `args` like bsvd_conv3x3: < 0 = bad argument.
 */
int64_t bsvd_workspace_bytes(const BsvdConvArgs *args);

/*
 * Steady-state streaming step as ONE submission (SURVEY.md §7.1 "hipGraph-capture one steady-state step"; replaces the
 * per-layer Python/torch dispatch under BSVD.feedin_one_element, bsvd_arch.py:485-488).
 *
 * bsvd_conv3x3_batch: validates and enqueues args[0..n-1] in order on `stream` (same semantics as n calls of
 * bsvd_conv3x3); stops at the first failing layer and returns its code (bsvd_last_error() names the index).
 *
 * Graph capture: the host brackets a batch with bsvd_graph_begin / bsvd_graph_end on a NON-default capture stream (nothing
 * executes while capturing), gets an executable graph handle and replays it with bsvd_graph_launch on any stream, once
 * per frame.  All device pointers are baked into the graph, so the host keeps every buffer of a step in fixed rings
 * (bsvd_amd/stream_plan.py).  bsvd_graph_fork / bsvd_graph_join make a second stream part of the capture so that two
 * independent layer chains (the two DenBlocks of consecutive pipeline steps) become parallel branches of one graph.
 * A graph handle owns no device memory; bsvd_graph_destroy releases it.  Capture mode is "relaxed": other threads of
 * the process are not restricted while a capture is open.
 */
int bsvd_conv3x3_batch(const BsvdConvArgs *args, int32_t n, void *stream);
int bsvd_graph_begin(void *capture_stream);
int bsvd_graph_fork(void *capture_stream, void *side_stream);
int bsvd_graph_join(void *capture_stream, void *side_stream);
int bsvd_graph_end(void *capture_stream, void **graph_exec, int32_t *num_nodes);
int bsvd_graph_abort(void *capture_stream);   /* ends a capture after a failed launch and discards it */
int bsvd_graph_launch(void *graph_exec, void *stream);
int bsvd_graph_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* BSVD_HIP_H */
