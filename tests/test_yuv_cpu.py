"""YUV 4:2:0 frame I/O (bsvd_yuv420_to_planar / bsvd_planar_to_yuv420, frame_io.yuv420_to_input / output_to_yuv420, pix_fmt of the
pipelines): what needs no device -- the numpy model's colour-bar codes, the frame size, every validation case of the two entry points with
its error text, the unchanged ABI version and BsvdConvArgs, and the pipelines' argument errors."""
import ctypes

import numpy as np
import pytest

import yuv_model as M

# limited-range (Y, Cb, Cr) of white, red, green, blue, black
BARS = {
    8: {"bt601": [(235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (16, 128, 128)],
        "bt709": [(235, 128, 128), (63, 102, 240), (173, 42, 26), (32, 240, 118), (16, 128, 128)],
        "bt2020": [(235, 128, 128), (74, 97, 240), (164, 47, 25), (29, 240, 119), (16, 128, 128)]},
    10: {"bt601": [(940, 512, 512), (326, 361, 960), (578, 215, 137), (164, 960, 439), (64, 512, 512)],
         "bt709": [(940, 512, 512), (250, 409, 960), (691, 167, 105), (127, 960, 471), (64, 512, 512)],
         "bt2020": [(940, 512, 512), (294, 387, 960), (658, 189, 100), (116, 960, 476), (64, 512, 512)]},
}
RGB = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
@pytest.mark.parametrize("chroma", ["nearest", "linear"])
def test_model_colour_bar_codes(bits, matrix, chroma):
    """The model encodes flat colour bars to the published limited-range codes, in float64 and in float32, and decodes them back."""
    for rgb, want in zip(RGB, BARS[bits][matrix]):
        x = np.broadcast_to(np.array(rgb, np.float64)[None, :, None, None], (1, 3, 4, 8)).copy()
        for dtype in (np.float64, np.float32):
            Y, Cb, Cr = M.encode(x, bits, matrix=matrix, full_range=False, chroma=chroma, dtype=dtype)
            assert (int(Y[0, 0, 0]), int(Cb[0, 0, 0]), int(Cr[0, 0, 0])) == want, (rgb, dtype)
            assert (Y == Y[0, 0, 0]).all() and (Cb == Cb[0, 0, 0]).all() and (Cr == Cr[0, 0, 0]).all()
        back = M.decode(Y, Cb, Cr, bits, matrix=matrix, full_range=False, chroma=chroma)
        # half a code of luma and half a code of chroma through a matrix entry of at most 2 (1 - Kb) < 1.9
        assert np.abs(back - x).max() < 1.5 / (219 * 2 ** (bits - 8))


def test_model_pack_unpack_round_trip():
    rs = np.random.RandomState(0)
    for pix_fmt, top, pitch, stride in (("nv12", 256, None, None), ("nv12", 256, 24, 24 * 12 + 7), ("p010", 1024, 40, 40 * 12 + 16)):
        Y, Cb, Cr = rs.randint(0, top, (2, 8, 12)), rs.randint(0, top, (2, 4, 6)), rs.randint(0, top, (2, 4, 6))
        buf = M.pack(Y, Cb, Cr, pix_fmt, pitch, stride, fill=0xA5, low_bits=rs.randint(0, 64, (2, 12, 12)))
        assert buf.shape == (2, stride or M.frame_bytes(8, 12, pix_fmt, pitch))
        y2, cb2, cr2, _ = M.unpack(buf, 8, 12, pix_fmt, pitch)
        assert np.array_equal(y2, Y) and np.array_equal(cb2, Cb) and np.array_equal(cr2, Cr)
        mask = M.sample_mask(2, 8, 12, pix_fmt, pitch, stride)
        assert mask.sum() == 2 * 8 * 12 * 3 // 2 * (2 if pix_fmt == "p010" else 1) and (buf[~mask] == 0xA5).all()


def test_frame_bytes():
    from bsvd_amd import _lib
    from bsvd_amd.frame_io import yuv420_frame_bytes
    lib = _lib.load()
    NV12, P010 = _lib.PIX_FMT["nv12"], _lib.PIX_FMT["p010"]
    assert lib.bsvd_yuv420_frame_bytes(1080, 1920, NV12, 0) == 1920 * 1080 * 3 // 2
    assert lib.bsvd_yuv420_frame_bytes(1080, 1920, P010, 0) == 2 * 1920 * 1080 * 3 // 2
    assert lib.bsvd_yuv420_frame_bytes(1080, 1920, NV12, 2048) == 2048 * 1080 * 3 // 2
    assert lib.bsvd_yuv420_frame_bytes(1080, 1920, P010, 4096) == 4096 * 1080 * 3 // 2
    assert lib.bsvd_yuv420_frame_bytes(4, 4, NV12, 5) == 5 * 6                     # NV12 pitches need no alignment
    for bad in ((0, 8, NV12, 0), (8, 0, NV12, 0), (-4, 8, NV12, 0), (6, 8, NV12, 0), (8, 10, NV12, 0), (8, 8, 2, 0), (8, 8, -1, 0),
                (8, 8, NV12, 7), (8, 8, P010, 15), (8, 8, P010, 17), (8, 8, NV12, -8)):
        assert lib.bsvd_yuv420_frame_bytes(*bad) == -1, bad
    assert yuv420_frame_bytes(1080, 1920, "nv12") == 1920 * 1080 * 3 // 2
    assert yuv420_frame_bytes(36, 52, "p010", 192) == 192 * 54
    for bad in ((8, 8, "yuyv"), (6, 8, "nv12"), (8, 8, "p010", 17)):
        with pytest.raises(ValueError):
            yuv420_frame_bytes(*bad)


def _desc(**kw):
    from bsvd_amd import _lib
    return _lib.BsvdYuvDesc(**{"pix_fmt": 0, "matrix": 1, "full_range": 0, "chroma": 1, **kw})


# (changes to a valid call, the words the error must contain): every case of the header's list
BAD = [
    (dict(yuv=None), "is NULL"),
    (dict(planar=None), "is NULL"),
    (dict(desc=None), "desc is NULL"),
    (dict(frames=0), "frames"),
    (dict(frames=-1), "frames"),
    (dict(H=0), "H = 0"),
    (dict(H=-8), "H = -8"),
    (dict(H=6), "H = 6"),
    (dict(W=0), "W = 0"),
    (dict(W=10), "W = 10"),
    (dict(d=dict(pix_fmt=2)), "pix_fmt"),
    (dict(d=dict(pix_fmt=-1)), "pix_fmt"),
    (dict(d=dict(matrix=3)), "matrix"),
    (dict(d=dict(full_range=2)), "full_range"),
    (dict(d=dict(chroma=2)), "chroma"),
    (dict(d=dict(reserved=1)), "reserved"),
    (dict(d=dict(row_pitch=11)), "row_pitch"),                                  # W = 12 samples
    (dict(d=dict(pix_fmt=1, row_pitch=22)), "row_pitch"),                       # 12 P010 samples are 24 bytes
    (dict(d=dict(pix_fmt=1, row_pitch=33)), "row_pitch"),                       # odd
    (dict(d=dict(pix_fmt=1), yuv=4097), "2-byte aligned"),
    (dict(d=dict(frame_stride=12 * 12 - 1)), "frame_stride"),                   # one tight 8 x 12 NV12 frame is 144 bytes
    (dict(d=dict(row_pitch=64, frame_stride=12 * 12)), "frame_stride"),         # ... and 768 with that pitch
    (dict(d=dict(pix_fmt=1, frame_stride=2 * 12 * 12 + 1)), "frame_stride"),    # P010 frames an odd number of bytes apart
    (dict(planar=4100), "16-byte aligned"),
]


@pytest.mark.parametrize("change,words", BAD)
def test_validation_names_the_argument(change, words):
    """Both entry points refuse each bad argument with -3 and say which one -- before any launch, without a device."""
    from bsvd_amd import _lib
    lib = _lib.load()
    change = dict(change)
    d = _desc(**change.pop("d", {}))
    a = dict(yuv=4096, planar=8192, frames=2, H=8, W=12, desc=ctypes.byref(d))
    a.update(change)
    rc = lib.bsvd_yuv420_to_planar(a["yuv"], a["planar"], a["frames"], a["H"], a["W"], a["desc"], 1, 0.1, None)
    assert rc == -3
    err = lib.bsvd_last_error().decode()
    assert err.startswith("bsvd_yuv420_to_planar: ") and words in err, err
    if "NULL" in words and "desc" not in words:
        assert ("src" if change.get("yuv", 1) is None else "dst") in err, err
    rc = lib.bsvd_planar_to_yuv420(a["planar"], a["yuv"], a["frames"], a["H"], a["W"], a["desc"], None)
    assert rc == -3
    err = lib.bsvd_last_error().decode()
    assert err.startswith("bsvd_planar_to_yuv420: ") and words in err, err
    if "NULL" in words and "desc" not in words:
        assert ("dst" if change.get("yuv", 1) is None else "src") in err, err


def test_validation_const_channels():
    from bsvd_amd import _lib
    lib = _lib.load()
    d = _desc()
    assert lib.bsvd_yuv420_to_planar(4096, 8192, 1, 8, 12, ctypes.byref(d), -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()


def test_abi_version_and_conv_args_unchanged():
    """The YUV entry points came without a new ABI version: discovered by symbol, BsvdConvArgs as it was."""
    from bsvd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 12 and lib.bsvd_abi_version() == 12
    assert ctypes.sizeof(_lib.BsvdConvArgs) == 272 == lib.bsvd_conv_args_size()
    for name in ("bsvd_yuv420_frame_bytes", "bsvd_yuv420_to_planar", "bsvd_planar_to_yuv420"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    D = _lib.BsvdYuvDesc
    assert ctypes.sizeof(D) == 32 and D.frame_stride.offset == 24 and D.row_pitch.offset == 16 and D.reserved.offset == 20


def test_frame_io_argument_errors():
    """Names and host-side checks come before the device is asked for."""
    import torch
    from bsvd_amd.frame_io import output_to_yuv420, yuv420_to_input
    buf = torch.zeros((1, 144), dtype=torch.uint8)
    for kw in (dict(pix_fmt="yv12"), dict(matrix="bt470"), dict(chroma="cubic"), dict(row_pitch=8)):
        with pytest.raises(ValueError):
            yuv420_to_input(buf, 8, 12, **kw)
    with pytest.raises(ValueError):
        yuv420_to_input(buf, 8, 10)
    with pytest.raises(ValueError):
        output_to_yuv420(torch.zeros((1, 3, 8, 12)))                # not on the device
    with pytest.raises(ValueError):
        output_to_yuv420(torch.zeros((1, 4, 8, 12)))


def test_pipeline_argument_errors():
    """pix_fmt and colour are checked when a pipeline is constructed, before its model or a device is touched; a frame's dtype and plane
    shape by ``fmt.geometry``, the first thing submit() / feed() call."""
    from bsvd_amd.pipeline import ClipPipeline, Colour, LiveStream, _pixel_format
    for cls in (ClipPipeline, LiveStream):
        with pytest.raises(ValueError, match="pix_fmt"):
            cls(None, pix_fmt="yuv444")
        with pytest.raises(ValueError, match="matrix"):
            cls(None, pix_fmt="nv12", colour={"matrix": "bt470"})
        with pytest.raises(ValueError, match="chroma"):
            cls(None, pix_fmt="p010", colour=Colour(chroma="cubic"))
        with pytest.raises(ValueError, match="colour"):
            cls(None, pix_fmt="nv12", colour={"gamma": 2.2})
        with pytest.raises(ValueError, match="colour"):
            cls(None, pix_fmt="rgb24", colour={"matrix": "bt709"})
    nv12, p010 = _pixel_format("nv12", None), _pixel_format("p010", {"row_pitch": 256, "width": 96})
    g = nv12.geometry(np.zeros((96, 96), np.uint8), clip=False)
    assert (g.h, g.w, g.staging, g.row_pitch) == (64, 96, (96 * 96,), None)
    g = p010.geometry(np.zeros((3, 96, 128), np.uint16), clip=True)
    assert (g.h, g.w, g.staging, g.row_pitch) == (64, 96, (3, 256 * 96), 256)
    for fmt, frame in ((nv12, np.zeros((96, 96), np.uint16)),             # wrong dtype for the format
                       (p010, np.zeros((96, 128), np.uint8)),
                       (nv12, np.zeros((64, 96, 3), np.uint8)),           # an RGB frame
                       (nv12, np.zeros((64, 96), np.uint8)),              # rows are not H * 3 / 2 with H % 4 == 0
                       (nv12, np.zeros((96, 98), np.uint8)),              # W % 4
                       (p010, np.zeros((96, 92), np.uint16)),             # rows shorter than the width
                       (p010, np.zeros((96, 160), np.uint16))):           # rows that are not colour.row_pitch
        with pytest.raises(ValueError):
            fmt.geometry(frame, clip=False)
    with pytest.raises(ValueError):
        nv12.geometry(np.zeros((96, 96), np.uint8), clip=True)             # one frame where a clip is expected
    rgb = _pixel_format("rgb24", None)
    assert rgb.geometry(np.zeros((2, 64, 96, 3), np.uint8), clip=True).staging == (2, 64, 96, 3)
    with pytest.raises(ValueError):
        rgb.geometry(np.zeros((96, 96), np.uint8), clip=False)
