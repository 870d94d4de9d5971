"""ctypes binding of libbsvd_hip.so (C ABI in include/bsvd_hip.h).

The library is built in-tree by ``bsvd_amd/csrc/build.sh`` (``__graft_entry__.build()``).  There is
no CPU fallback: if the shared object is missing or a HIP device is absent the product path raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSVD_HIP_LIB") or os.path.join(_HERE, "libbsvd_hip.so")   # env override: A/B tuning builds

ABI_VERSION = 12
BSVD_F32, BSVD_F16X3, BSVD_F16 = 0, 2, 3       # (1 is retired: the library refuses it)
ACT = {"none": 0, "relu": 1, "relu6": 2}
EPI_PLAIN, EPI_PS_ADD, EPI_RESID = 0, 1, 2
BUILD_MEASURE = 1            # bsvd_build_info(): a -DBSVD_MEASURE build (tools/build_measure.sh), never the in-tree product library

EXPORTS = ("bsvd_abi_version", "bsvd_conv_args_size", "bsvd_build_info", "bsvd_last_error", "bsvd_conv3x3", "bsvd_conv3x3_variant", "bsvd_packed_weight_elems", "bsvd_pack_weights",
           "bsvd_packed_head_weight_bytes", "bsvd_pack_head_weights", "bsvd_packed_wino_weight_elems", "bsvd_pack_weights_wino",
           "bsvd_nchw_to_nhwc", "bsvd_nhwc_to_nchw", "bsvd_halo_pack", "bsvd_halo_unpack", "bsvd_workspace_bytes",
           "bsvd_u8_to_planar", "bsvd_planar_to_u8", "bsvd_conv3x3_batch", "bsvd_graph_begin", "bsvd_graph_fork",
           "bsvd_graph_join", "bsvd_graph_end", "bsvd_graph_abort", "bsvd_graph_launch", "bsvd_graph_destroy",
           "bsvd_v_frame_elems", "bsvd_v_groups", "bsvd_to_v",
           "bsvd_yuv420_frame_bytes", "bsvd_yuv420_to_planar", "bsvd_planar_to_yuv420",
           "bsvd_u8_to_planar_pad", "bsvd_planar_to_u8_crop", "bsvd_yuv420_picture_bytes", "bsvd_yuv420_to_planar_pad",
           "bsvd_planar_to_yuv420_crop",
           "bsvd_yuv_frame_bytes", "bsvd_yuv_to_planar", "bsvd_planar_to_yuv", "bsvd_yuv_to_planar_pad", "bsvd_planar_to_yuv_crop",
           "bsvd_sigma_workspace_bytes", "bsvd_estimate_sigma", "bsvd_fill_sigma_plane",
           "bsvd_scene_grid", "bsvd_scene_diff",
           "bsvd_rgb_frame_bytes", "bsvd_rgb_to_planar", "bsvd_planar_to_rgb",
           "bsvd_blend_planar", "bsvd_planar_to_yuv420_crop_d", "bsvd_planar_to_yuv_crop_d", "bsvd_planar_to_rgb_d",
           "bsvd_nlf_workspace_bytes", "bsvd_estimate_nlf", "bsvd_finish_nlf", "bsvd_fill_nlf_plane",
           "bsvd_vst_build", "bsvd_vst_forward", "bsvd_vst_inverse",
           "bsvd_grain_stats_bytes", "bsvd_grain_stats", "bsvd_grain_apply")
PIX_FMT = {"nv12": 0, "p010": 1}
MATRIX = {"bt601": 0, "bt709": 1, "bt2020": 2}
CHROMA = {"nearest": 0, "linear": 1}
DITHER = {None: 0, "ordered": 1, "random": 2}           # BSVD_DITHER_*
DITHER_NONE, DITHER_ORDERED, DITHER_RANDOM = 0, 1, 2
# Kr, Kg, Kb of the matrices, as the encoders make them (frame_yuv.hip): Kg = 1 - Kr - Kb in double
LUMA_WEIGHTS = {name: (kr, 1.0 - kr - kb, kb) for name, (kr, kb) in (("bt601", (0.299, 0.114)), ("bt709", (0.2126, 0.0722)), ("bt2020", (0.2627, 0.0593)))}
SUB_420, SUB_422, SUB_444 = 0, 1, 2
LAYOUT_PLANAR, LAYOUT_SEMIPLANAR, LAYOUT_UYVY, LAYOUT_YUYV = 0, 1, 2, 3
SIGMA_BINS = 4096             # bins of bsvd_estimate_sigma's histogram: 1 / 4096 of |r| each
# the scale from the median bin to sigma, 1 / (4096 * 6 * 0.6744897501960817) (frame_sigma_items.h, SIGMA_K), and where the estimate saturates
SIGMA_K = float.fromhex("0x1.fa0fc23747344p-15")
SIGMA_MAX = SIGMA_BINS * SIGMA_K
# bsvd_estimate_nlf: levels of the noise-level curve, bins per level (1 / 1024 of |r| each: NLF_BINS * NLF_K = SIGMA_MAX), samples a level needs
NLF_LEVELS, NLF_BINS, NLF_MIN_COUNT = 16, 1024, 512
NLF_K = 4 * SIGMA_K
# bsvd_vst_build: a table set is G[0 .. 1024] at 0, sigma' at VST_SIGMA_AT, two zeros, R[0 .. 1023] at VST_R_AT; the default noise floor
VST_KNOTS = 1025
VST_SIGMA_AT, VST_R_AT = VST_KNOTS, VST_KNOTS + 3
VST_TABLE_FLOATS = VST_R_AT + VST_KNOTS - 1
VST_FLOOR = 0.5 / 255
VST_FLOOR_MIN = 2.0 ** -10
# bsvd_grain_stats: a frame's 256 int64 are N[16] at 0, sum q_k at GRAIN_S1_AT + 16 k + l, sum q_k^2 at GRAIN_S2_AT + 16 k + l, the lag
# products A[k][lag] at GRAIN_A_AT + 46 k + lag; q = noise * GRAIN_QSCALE; bsvd_grain_apply: templates [3][GRAIN_TMPL][GRAIN_TMPL]
GRAIN_LEVELS, GRAIN_LAGS, GRAIN_TAPS, GRAIN_STATS = 16, 46, 24, 256
GRAIN_N_AT, GRAIN_S1_AT, GRAIN_S2_AT, GRAIN_A_AT = 0, 16, 64, 112
GRAIN_QSCALE, GRAIN_TMPL, GRAIN_MIN_COUNT = 4096.0, 128, 512
# the surfaces of bsvd_yuv_to_planar / bsvd_planar_to_yuv, by ffmpeg's names: (subsampling, layout, bits, high_bits).  PIX_FMT above stays
# the table of the bsvd_yuv420_* entry points.
YUV_FORMATS = {
    "yuv420p": (SUB_420, LAYOUT_PLANAR, 8, 0), "yuv420p10le": (SUB_420, LAYOUT_PLANAR, 10, 0),
    "uyvy422": (SUB_422, LAYOUT_UYVY, 8, 0), "yuyv422": (SUB_422, LAYOUT_YUYV, 8, 0),
    "nv16": (SUB_422, LAYOUT_SEMIPLANAR, 8, 0), "p210le": (SUB_422, LAYOUT_SEMIPLANAR, 10, 1),
    "yuv422p": (SUB_422, LAYOUT_PLANAR, 8, 0), "yuv422p10le": (SUB_422, LAYOUT_PLANAR, 10, 0),
    "yuv444p": (SUB_444, LAYOUT_PLANAR, 8, 0), "yuv444p10le": (SUB_444, LAYOUT_PLANAR, 10, 0),
}
RGB_PACKED, RGB_PACKED_X2_10, RGB_PLANAR = 0, 1, 2
FOURTH_NONE, FOURTH_ALPHA, FOURTH_FILLER = 0, 1, 2


def _rgb_formats():
    """the surfaces of bsvd_rgb_to_planar / bsvd_planar_to_rgb, by ffmpeg's names: (layout, components, bits, pos of R G B fourth, fourth)"""
    t = {}
    for name in ("rgb24", "bgr24", "rgba", "bgra", "argb", "abgr", "rgb0", "bgr0", "0rgb", "0bgr"):
        order = name[:-2] if name.endswith("24") else name
        fourth = FOURTH_ALPHA if "a" in order else FOURTH_FILLER if "0" in order else FOURTH_NONE
        pos = tuple(order.index(c) for c in "rgb") + ((order.index("a" if fourth == FOURTH_ALPHA else "0"),) if fourth else (0,))
        t[name] = (RGB_PACKED, len(order), 8, pos, fourth)
    t["rgb48le"] = (RGB_PACKED, 3, 16, (0, 1, 2, 0), FOURTH_NONE)
    t["bgr48le"] = (RGB_PACKED, 3, 16, (2, 1, 0, 0), FOURTH_NONE)
    t["rgba64le"] = (RGB_PACKED, 4, 16, (0, 1, 2, 3), FOURTH_ALPHA)
    t["bgra64le"] = (RGB_PACKED, 4, 16, (2, 1, 0, 3), FOURTH_ALPHA)
    t["x2rgb10le"] = (RGB_PACKED_X2_10, 3, 10, (2, 1, 0, 0), FOURTH_NONE)      # (msb) 2 X | R | G | B (lsb): B is field 0
    t["x2bgr10le"] = (RGB_PACKED_X2_10, 3, 10, (0, 1, 2, 0), FOURTH_NONE)
    for bits, suffix in ((8, ""), (10, "10le"), (12, "12le"), (16, "16le")):       # plane order G, B, R, (A)
        t["gbrp" + suffix] = (RGB_PLANAR, 3, bits, (2, 0, 1, 0), FOURTH_NONE)
        t["gbrap" + suffix] = (RGB_PLANAR, 4, bits, (2, 0, 1, 3), FOURTH_ALPHA)
    return t


RGB_FORMATS = _rgb_formats()


class BsvdConvArgs(ctypes.Structure):
    """Mirror of ``struct BsvdConvArgs`` (include/bsvd_hip.h) -- keep field order in sync."""
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("x_frame_stride", ctypes.c_int64),
        ("halo_prev", ctypes.c_void_p),
        ("halo_next", ctypes.c_void_p),
        ("halo_prev_pstride", ctypes.c_int32), ("halo_prev_coff", ctypes.c_int32),
        ("halo_next_pstride", ctypes.c_int32), ("halo_next_coff", ctypes.c_int32),
        ("fold", ctypes.c_int32),
        ("w_packed", ctypes.c_void_p),
        ("bias_packed", ctypes.c_void_p),
        ("extra", ctypes.c_void_p),
        ("extra_frame_stride", ctypes.c_int64),
        ("extra_pstride", ctypes.c_int32),
        ("extra_cstride", ctypes.c_int32),
        ("resid_ch", ctypes.c_int32),
        ("y", ctypes.c_void_p),
        ("y_frame_stride", ctypes.c_int64),
        ("frames", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32),
        ("stride", ctypes.c_int32),
        ("act", ctypes.c_int32), ("epilogue", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("x_planar_ch", ctypes.c_int32), ("y_planar_ch", ctypes.c_int32), ("y_clamp", ctypes.c_int32),
        ("y_lo", ctypes.c_float), ("y_hi", ctypes.c_float),
        ("extra_split", ctypes.c_int32),
        ("tile_order", ctypes.c_int32),
        ("head_w_packed", ctypes.c_void_p),
        ("head_bias", ctypes.c_void_p),
        ("w_wino_packed", ctypes.c_void_p),
        ("wino_m", ctypes.c_int32),
        ("fat_min_wgs", ctypes.c_int32),
        ("pre_w_packed", ctypes.c_void_p),
        ("pre_bias", ctypes.c_void_p),
        ("pre_cin", ctypes.c_int32), ("pre_act", ctypes.c_int32),
        ("x_f32", ctypes.c_int32), ("y_f32", ctypes.c_int32),
        ("x_v", ctypes.c_int32), ("y_v", ctypes.c_int32),
        ("out_scale", ctypes.c_float), ("head_out_scale", ctypes.c_float), ("pre_out_scale", ctypes.c_float),
    ]


class BsvdYuvDesc(ctypes.Structure):
    """Mirror of ``struct BsvdYuvDesc`` (include/bsvd_hip.h)."""
    _fields_ = [("pix_fmt", ctypes.c_int32), ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32), ("chroma", ctypes.c_int32),
                ("row_pitch", ctypes.c_int32), ("reserved", ctypes.c_int32), ("frame_stride", ctypes.c_int64)]


class BsvdYuvSurface(ctypes.Structure):
    """Mirror of ``struct BsvdYuvSurface`` (include/bsvd_hip.h)."""
    _fields_ = [("subsampling", ctypes.c_int32), ("layout", ctypes.c_int32), ("bits", ctypes.c_int32), ("high_bits", ctypes.c_int32),
                ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32), ("chroma", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("pitch", ctypes.c_int32 * 3), ("reserved1", ctypes.c_int32), ("offset", ctypes.c_int64 * 3),
                ("frame_stride", ctypes.c_int64), ("reserved2", ctypes.c_int64)]


class BsvdRgbSurface(ctypes.Structure):
    """Mirror of ``struct BsvdRgbSurface`` (include/bsvd_hip.h)."""
    _fields_ = [("layout", ctypes.c_int32), ("components", ctypes.c_int32), ("bits", ctypes.c_int32), ("pos", ctypes.c_int32 * 4),
                ("fourth", ctypes.c_int32), ("full_range", ctypes.c_int32), ("pitch", ctypes.c_int32 * 4), ("reserved0", ctypes.c_int32),
                ("offset", ctypes.c_int64 * 4), ("frame_stride", ctypes.c_int64), ("reserved", ctypes.c_int64)]


class BsvdDither(ctypes.Structure):
    """Mirror of ``struct BsvdDither`` (include/bsvd_hip.h)."""
    _fields_ = [("mode", ctypes.c_int32), ("seed", ctypes.c_uint32), ("frame0", ctypes.c_int64), ("reserved", ctypes.c_int64)]


class BsvdLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Loads the shared object and declares prototypes.  Raises BsvdLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BsvdLibraryError(
            "libbsvd_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "bsvd_amd/csrc/build.sh -- bsvd_amd has no CPU fallback." % LIB_PATH)
    if os.environ.get("BSVD_HIP_LIB"):
        import sys
        print("bsvd_amd: BSVD_HIP_LIB override -- loading %s instead of the in-tree libbsvd_hip.so" % LIB_PATH, file=sys.stderr)
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.bsvd_abi_version.restype = ctypes.c_int
    lib.bsvd_abi_version.argtypes = []
    lib.bsvd_conv_args_size.restype = ctypes.c_int
    lib.bsvd_conv_args_size.argtypes = []
    lib.bsvd_build_info.restype = ctypes.c_int
    lib.bsvd_build_info.argtypes = []
    lib.bsvd_last_error.restype = ctypes.c_char_p
    lib.bsvd_last_error.argtypes = []
    lib.bsvd_conv3x3.restype = ctypes.c_int
    lib.bsvd_conv3x3.argtypes = [ctypes.POINTER(BsvdConvArgs), vp]
    lib.bsvd_conv3x3_variant.restype = ctypes.c_int
    lib.bsvd_conv3x3_variant.argtypes = [ctypes.POINTER(BsvdConvArgs), ctypes.c_char_p, i32]
    lib.bsvd_packed_weight_elems.restype = i64
    lib.bsvd_packed_weight_elems.argtypes = [i32, i32]
    lib.bsvd_pack_weights.restype = ctypes.c_int
    lib.bsvd_pack_weights.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.bsvd_packed_wino_weight_elems.restype = i64
    lib.bsvd_packed_wino_weight_elems.argtypes = [i32, i32, i32]
    lib.bsvd_pack_weights_wino.restype = ctypes.c_int
    lib.bsvd_pack_weights_wino.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.bsvd_packed_head_weight_bytes.restype = i64
    lib.bsvd_packed_head_weight_bytes.argtypes = [i32]
    lib.bsvd_pack_head_weights.restype = ctypes.c_int
    lib.bsvd_pack_head_weights.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.bsvd_nchw_to_nhwc.restype = ctypes.c_int
    lib.bsvd_nchw_to_nhwc.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.bsvd_nhwc_to_nchw.restype = ctypes.c_int
    lib.bsvd_nhwc_to_nchw.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp]
    lib.bsvd_u8_to_planar.restype = ctypes.c_int
    lib.bsvd_u8_to_planar.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.bsvd_planar_to_u8.restype = ctypes.c_int
    lib.bsvd_planar_to_u8.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.bsvd_halo_pack.restype = ctypes.c_int
    lib.bsvd_halo_pack.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.bsvd_halo_unpack.restype = ctypes.c_int
    lib.bsvd_halo_unpack.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.bsvd_conv3x3_batch.restype = ctypes.c_int
    lib.bsvd_conv3x3_batch.argtypes = [ctypes.POINTER(BsvdConvArgs), i32, vp]
    for fn, at in (("bsvd_graph_begin", [vp]), ("bsvd_graph_fork", [vp, vp]), ("bsvd_graph_join", [vp, vp]),
                   ("bsvd_graph_end", [vp, ctypes.POINTER(vp), ctypes.POINTER(i32)]), ("bsvd_graph_abort", [vp]),
                   ("bsvd_graph_launch", [vp, vp]), ("bsvd_graph_destroy", [vp])):
        getattr(lib, fn).restype = ctypes.c_int
        getattr(lib, fn).argtypes = at
    lib.bsvd_v_frame_elems.restype = i64
    lib.bsvd_v_frame_elems.argtypes = [i32, i32, i32, i32]
    lib.bsvd_v_groups.restype = i32
    lib.bsvd_v_groups.argtypes = [i32, i32]
    lib.bsvd_to_v.restype = ctypes.c_int
    lib.bsvd_to_v.argtypes = [vp, i64, i32, vp, i64, i32, i32, i32, i32, i32, vp]
    lib.bsvd_yuv420_frame_bytes.restype = i64
    lib.bsvd_yuv420_frame_bytes.argtypes = [i32, i32, i32, i32]
    lib.bsvd_yuv420_to_planar.restype = ctypes.c_int
    lib.bsvd_yuv420_to_planar.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(BsvdYuvDesc), i32, f32, vp]
    lib.bsvd_planar_to_yuv420.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv420.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(BsvdYuvDesc), vp]
    lib.bsvd_u8_to_planar_pad.restype = ctypes.c_int
    lib.bsvd_u8_to_planar_pad.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.bsvd_planar_to_u8_crop.restype = ctypes.c_int
    lib.bsvd_planar_to_u8_crop.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.bsvd_yuv420_picture_bytes.restype = i64
    lib.bsvd_yuv420_picture_bytes.argtypes = [i32, i32, i32, i32]
    lib.bsvd_yuv420_to_planar_pad.restype = ctypes.c_int
    lib.bsvd_yuv420_to_planar_pad.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.POINTER(BsvdYuvDesc), i32, f32, vp]
    lib.bsvd_planar_to_yuv420_crop.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv420_crop.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.POINTER(BsvdYuvDesc), vp]
    surf = ctypes.POINTER(BsvdYuvSurface)
    lib.bsvd_yuv_frame_bytes.restype = i64
    lib.bsvd_yuv_frame_bytes.argtypes = [i32, i32, surf]
    lib.bsvd_yuv_to_planar.restype = ctypes.c_int
    lib.bsvd_yuv_to_planar.argtypes = [vp, vp, i32, i32, i32, surf, i32, f32, vp]
    lib.bsvd_planar_to_yuv.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv.argtypes = [vp, vp, i32, i32, i32, surf, vp]
    lib.bsvd_yuv_to_planar_pad.restype = ctypes.c_int
    lib.bsvd_yuv_to_planar_pad.argtypes = [vp, vp, i32, i32, i32, i32, i32, surf, i32, f32, vp]
    lib.bsvd_planar_to_yuv_crop.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv_crop.argtypes = [vp, vp, i32, i32, i32, i32, i32, surf, vp]
    lib.bsvd_sigma_workspace_bytes.restype = i64
    lib.bsvd_sigma_workspace_bytes.argtypes = [i32]
    lib.bsvd_estimate_sigma.restype = ctypes.c_int
    lib.bsvd_estimate_sigma.argtypes = [vp, i32, i32, i32, i32, i32, i32, i64, f32, f32, f32, vp, vp, vp]
    lib.bsvd_fill_sigma_plane.restype = ctypes.c_int
    lib.bsvd_fill_sigma_plane.argtypes = [vp, i32, i32, i32, i32, i64, vp, vp]
    lib.bsvd_nlf_workspace_bytes.restype = i64
    lib.bsvd_nlf_workspace_bytes.argtypes = [i32]
    lib.bsvd_estimate_nlf.restype = ctypes.c_int
    lib.bsvd_estimate_nlf.argtypes = [vp, i32, i32, i32, i32, i32, i64, f32, f32, f32, i32, vp, vp, vp]
    lib.bsvd_finish_nlf.restype = ctypes.c_int
    lib.bsvd_finish_nlf.argtypes = [vp, i32, f32, f32, f32, i32, vp, vp]
    lib.bsvd_fill_nlf_plane.restype = ctypes.c_int
    lib.bsvd_fill_nlf_plane.argtypes = [vp, i32, i32, i32, i32, i64, vp, vp]
    lib.bsvd_vst_build.restype = ctypes.c_int
    lib.bsvd_vst_build.argtypes = [vp, i32, f32, vp, vp]
    lib.bsvd_vst_forward.restype = ctypes.c_int
    lib.bsvd_vst_forward.argtypes = [vp, i32, i32, i32, i64, i32, vp, i64, vp]
    lib.bsvd_vst_inverse.restype = ctypes.c_int
    lib.bsvd_vst_inverse.argtypes = [vp, i64, i32, i32, i32, vp, i64, vp]
    lib.bsvd_grain_stats_bytes.restype = ctypes.c_int64
    lib.bsvd_grain_stats_bytes.argtypes = [i32]
    lib.bsvd_grain_stats.restype = ctypes.c_int
    lib.bsvd_grain_stats.argtypes = [vp, i64, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.bsvd_grain_apply.restype = ctypes.c_int
    lib.bsvd_grain_apply.argtypes = [vp, i64, i32, i32, i32, vp, vp, f32, vp, f32, ctypes.c_uint32, i64, vp]
    lib.bsvd_scene_grid.restype = ctypes.c_int
    lib.bsvd_scene_grid.argtypes = [vp, i32, i32, i32, i32, i32, i64, vp, vp]
    lib.bsvd_scene_diff.restype = ctypes.c_int
    lib.bsvd_scene_diff.argtypes = [vp, vp, i32, i32, vp, vp]
    rgb = ctypes.POINTER(BsvdRgbSurface)
    lib.bsvd_rgb_frame_bytes.restype = i64
    lib.bsvd_rgb_frame_bytes.argtypes = [i32, i32, rgb]
    lib.bsvd_rgb_to_planar.restype = ctypes.c_int
    lib.bsvd_rgb_to_planar.argtypes = [vp, vp, i32, i32, i32, i32, i32, rgb, vp, i32, f32, vp]
    lib.bsvd_planar_to_rgb.restype = ctypes.c_int
    lib.bsvd_planar_to_rgb.argtypes = [vp, vp, i32, i32, i32, i32, i32, rgb, vp, vp]
    dith = ctypes.POINTER(BsvdDither)
    lib.bsvd_blend_planar.restype = ctypes.c_int
    lib.bsvd_blend_planar.argtypes = [vp, i64, vp, i64, i32, i32, i32, f32, f32, ctypes.POINTER(f32), vp]
    lib.bsvd_planar_to_yuv420_crop_d.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv420_crop_d.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.POINTER(BsvdYuvDesc), dith, vp]
    lib.bsvd_planar_to_yuv_crop_d.restype = ctypes.c_int
    lib.bsvd_planar_to_yuv_crop_d.argtypes = [vp, vp, i32, i32, i32, i32, i32, surf, dith, vp]
    lib.bsvd_planar_to_rgb_d.restype = ctypes.c_int
    lib.bsvd_planar_to_rgb_d.argtypes = [vp, vp, i32, i32, i32, i32, i32, rgb, vp, dith, vp]
    lib.bsvd_workspace_bytes.restype = i64
    lib.bsvd_workspace_bytes.argtypes = [ctypes.POINTER(BsvdConvArgs)]
    if lib.bsvd_abi_version() != ABI_VERSION:
        raise BsvdLibraryError("libbsvd_hip.so ABI version %d, expected %d" % (lib.bsvd_abi_version(), ABI_VERSION))
    if lib.bsvd_conv_args_size() != ctypes.sizeof(BsvdConvArgs):
        raise BsvdLibraryError("BsvdConvArgs layout mismatch: library %d bytes, binding %d bytes"
                               % (lib.bsvd_conv_args_size(), ctypes.sizeof(BsvdConvArgs)))
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    lib = load()
    if rc < 0:
        raise ValueError("%s: %s (rc=%d)" % (what, lib.bsvd_last_error().decode(), rc))
    raise BsvdLibraryError("%s: HIP error %d" % (what, rc))
