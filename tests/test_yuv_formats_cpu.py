"""The planar, 4:2:2 and 4:4:4 YUV surfaces (bsvd_yuv_frame_bytes, bsvd_yuv_to_planar / bsvd_planar_to_yuv, their _pad / _crop forms,
frame_io.yuv_to_input / output_to_yuv, the pipelines' ten new pix_fmt names): what needs no device -- the numpy model's colour-bar codes
and byte layouts, the frame size against the model, the struct's size and offsets, every validation case of the five entry points with
its error text, the unchanged ABI version / BsvdConvArgs / BsvdYuvDesc, the names that stay refused, and the geometry of the 1-D frames."""
import ctypes

import numpy as np
import pytest

import yuv_surface_model as S

NAMES = sorted(S.FORMATS)
# limited-range (Y, Cb, Cr) of white, red, green, blue, black: the published codes
BARS = {
    8: {"bt601": [(235, 128, 128), (81, 90, 240), (145, 54, 34), (41, 240, 110), (16, 128, 128)],
        "bt709": [(235, 128, 128), (63, 102, 240), (173, 42, 26), (32, 240, 118), (16, 128, 128)],
        "bt2020": [(235, 128, 128), (74, 97, 240), (164, 47, 25), (29, 240, 119), (16, 128, 128)]},
    10: {"bt601": [(940, 512, 512), (326, 361, 960), (578, 215, 137), (164, 960, 439), (64, 512, 512)],
         "bt709": [(940, 512, 512), (250, 409, 960), (691, 167, 105), (127, 960, 471), (64, 512, 512)],
         "bt2020": [(940, 512, 512), (294, 387, 960), (658, 189, 100), (116, 960, 476), (64, 512, 512)]},
}
RGB = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _surface(pix_fmt, **kw):
    from bsvd_amd import _lib
    sub, layout, bits, high = _lib.YUV_FORMATS[pix_fmt]
    pitch, offset = kw.pop("pitch", (0, 0, 0)), kw.pop("offset", (0, 0, 0))
    s = _lib.BsvdYuvSurface(**{"subsampling": sub, "layout": layout, "bits": bits, "high_bits": high, "matrix": 1, "full_range": 0,
                               "chroma": 1, **kw})
    s.pitch[:] = pitch
    s.offset[:] = offset
    return s


def test_binding_names_the_ten_formats_like_the_model():
    from bsvd_amd import _lib
    assert sorted(_lib.YUV_FORMATS) == NAMES and len(NAMES) == 10
    subs = {_lib.SUB_420: 420, _lib.SUB_422: 422, _lib.SUB_444: 444}
    lays = {_lib.LAYOUT_PLANAR: "planar", _lib.LAYOUT_SEMIPLANAR: "semi", _lib.LAYOUT_UYVY: "uyvy", _lib.LAYOUT_YUYV: "yuyv"}
    for n in NAMES:
        sub, layout, bits, high = _lib.YUV_FORMATS[n]
        assert S.FORMATS[n] == S.Format(subs[sub], lays[layout], bits, bool(high)), n
    assert _lib.PIX_FMT == {"nv12": 0, "p010": 1}                      # the table of the bsvd_yuv420_* entry points is what it was


@pytest.mark.parametrize("pix_fmt", [n for n in NAMES if "420" not in n])
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
@pytest.mark.parametrize("chroma", ["nearest", "linear"])
def test_model_colour_bar_codes(pix_fmt, matrix, chroma):
    """The model encodes flat colour bars to the published limited-range codes at 4:2:2 and 4:4:4, in float64 and in float32, and decodes
    them back."""
    bits = S.FORMATS[pix_fmt].bits
    for rgb, want in zip(RGB, BARS[bits][matrix]):
        x = np.broadcast_to(np.array(rgb, np.float64)[None, :, None, None], (1, 3, 4, 8)).copy()
        for dtype in (np.float64, np.float32):
            Y, Cb, Cr = S.encode(x, pix_fmt, matrix=matrix, full_range=False, chroma=chroma, dtype=dtype)
            assert Cb.shape == (1,) + S.chroma_shape(4, 8, S.FORMATS[pix_fmt].sub)
            assert (int(Y[0, 0, 0]), int(Cb[0, 0, 0]), int(Cr[0, 0, 0])) == want, (rgb, dtype)
            assert (Y == Y[0, 0, 0]).all() and (Cb == Cb[0, 0, 0]).all() and (Cr == Cr[0, 0, 0]).all()
        back = S.decode(Y, Cb, Cr, pix_fmt, matrix=matrix, full_range=False, chroma=chroma)
        # half a code of luma and half a code of chroma through a matrix entry of at most 2 (1 - Kb) < 1.9
        assert np.abs(back - x).max() < 1.5 / (219 * 2 ** (bits - 8))


def test_model_422_filters_follow_the_formulas():
    c = np.array([[[10, 20, 60]]])
    assert S.upsample(c, 422, "nearest", np.float64).tolist() == [[[10, 10, 20, 20, 60, 60]]]
    assert S.upsample(c, 422, "linear", np.float64).tolist() == [[[10, 15, 20, 40, 60, 60]]]         # the last odd column clamps
    x = np.array([[[4.0, 8.0, 16.0, 32.0, 64.0, 128.0]]])
    assert S.downsample(x, 422, "nearest", np.float64).tolist() == [[[6.0, 24.0, 96.0]]]
    assert S.downsample(x, 422, "linear", np.float64).tolist() == [[[(4 + 8 + 8) / 4, (8 + 32 + 32) / 4, (32 + 128 + 128) / 4]]]
    assert S.downsample(x, 444, "linear", np.float64) is x


@pytest.mark.parametrize("pix_fmt", NAMES)
def test_model_pack_unpack_round_trip(pix_fmt):
    """tight and pitched with offsets: the codes come back, junk in the ignored bits does not, every other byte is the fill"""
    f = S.FORMATS[pix_fmt]
    rs = np.random.RandomState(0)
    H, W, T, top = 8, 12, 2, 2 ** f.bits
    ch, cw = S.chroma_shape(H, W, f.sub)
    Y, Cb, Cr = rs.randint(0, top, (T, H, W)), rs.randint(0, top, (T, ch, cw)), rs.randint(0, top, (T, ch, cw))
    n = len(S.planes(H, W, pix_fmt))
    sample_bytes = (H * W + 2 * ch * cw) * (2 if f.bits > 8 else 1)
    assert S.frame_bytes(H, W, pix_fmt) == sample_bytes
    tight = [rb for _, rb in S.planes(H, W, pix_fmt)]
    pitches = [rb + 6 + 2 * i for i, rb in enumerate(tight)]
    offsets = [4] + [0, pitches[0] * H + 4 + pitches[1] * ch + 10][:n - 1] if n > 1 else [4]
    for P, O, stride in ((None, None, None), (pitches, offsets, None), (pitches, offsets, S.frame_bytes(H, W, pix_fmt, pitches, offsets) + 6)):
        buf = S.pack(Y, Cb, Cr, pix_fmt, P, O, stride, fill=0xA5, junk=rs)
        assert buf.shape == (T, stride or S.frame_bytes(H, W, pix_fmt, P, O))
        y2, cb2, cr2, ignored = S.unpack(buf, H, W, pix_fmt, P, O)
        assert np.array_equal(y2, Y) and np.array_equal(cb2, Cb) and np.array_equal(cr2, Cr)
        assert (ignored != 0) == (f.bits > 8)
        mask = S.sample_mask(T, H, W, pix_fmt, P, O, stride)
        assert mask.sum() == T * sample_bytes and (buf[~mask] == 0xA5).all()
    if f.layout == "uyvy":
        assert S.pack(Y, Cb, Cr, pix_fmt)[0, :4].tolist() == [Cb[0, 0, 0], Y[0, 0, 0], Cr[0, 0, 0], Y[0, 0, 1]]
    if f.layout == "yuyv":
        assert S.pack(Y, Cb, Cr, pix_fmt)[0, :4].tolist() == [Y[0, 0, 0], Cb[0, 0, 0], Y[0, 0, 1], Cr[0, 0, 0]]
    if pix_fmt == "p210le":
        assert S.pack(Y, Cb, Cr, pix_fmt).view("<u2")[0, 0] == Y[0, 0, 0] << 6
    if pix_fmt == "yuv422p10le":
        assert S.pack(Y, Cb, Cr, pix_fmt).view("<u2")[0, 0] == Y[0, 0, 0]


@pytest.mark.parametrize("pix_fmt", NAMES)
def test_frame_bytes_against_the_model(pix_fmt):
    from bsvd_amd import _lib
    from bsvd_amd.frame_io import yuv_frame_bytes, yuv_planes
    lib = _lib.load()
    f = S.FORMATS[pix_fmt]
    sizes = [(1080, 1920), (4, 4), (36, 52)] + {420: [(6, 10)], 422: [(5, 10)], 444: [(5, 7), (2, 2)]}[f.sub]
    for H, W in sizes:
        pl = S.planes(H, W, pix_fmt)
        assert yuv_planes(pix_fmt) == len(pl)
        s = _surface(pix_fmt)
        assert lib.bsvd_yuv_frame_bytes(H, W, ctypes.byref(s)) == S.frame_bytes(H, W, pix_fmt) == yuv_frame_bytes(H, W, pix_fmt)
        pitches = [rb + 64 + 2 * i for i, (_, rb) in enumerate(pl)]
        want = S.frame_bytes(H, W, pix_fmt, pitches)
        assert want == sum(p * rows for p, (rows, _) in zip(pitches, pl))
        s = _surface(pix_fmt, pitch=tuple(pitches + [0] * (3 - len(pl))))
        assert lib.bsvd_yuv_frame_bytes(H, W, ctypes.byref(s)) == want == yuv_frame_bytes(H, W, pix_fmt, pitches)
        offsets = [16] + [0, 16 + sum(p * rows for p, (rows, _) in zip(pitches[:2], pl[:2])) + 32][:len(pl) - 1]
        want = S.frame_bytes(H, W, pix_fmt, pitches, offsets)
        assert want == 16 + sum(p * rows for p, (rows, _) in zip(pitches, pl)) + (32 if len(pl) == 3 else 0)
        assert yuv_frame_bytes(H, W, pix_fmt, pitches, offsets) == want
    bad = {420: [(5, 8), (6, 7), (0, 8)], 422: [(5, 7), (1, 8), (4, 0)], 444: [(1, 5), (5, 1), (-4, 4)]}[f.sub]
    for H, W in bad:
        assert lib.bsvd_yuv_frame_bytes(H, W, ctypes.byref(_surface(pix_fmt))) == -1, (H, W)
        with pytest.raises(ValueError):
            yuv_frame_bytes(H, W, pix_fmt)
    assert lib.bsvd_yuv_frame_bytes(8, 8, None) == -1
    assert lib.bsvd_yuv_frame_bytes(8, 8, ctypes.byref(_surface(pix_fmt, pitch=(7, 0, 0)))) == -1
    assert lib.bsvd_yuv_frame_bytes(8, 8, ctypes.byref(_surface(pix_fmt, reserved2=1))) == -1
    with pytest.raises(ValueError):
        yuv_frame_bytes(8, 8, pix_fmt, [7])
    with pytest.raises(ValueError):
        yuv_frame_bytes(8, 8, pix_fmt, [64, 64, 64, 64])


def test_struct_and_abi():
    """BsvdYuvSurface is 88 bytes with the header's offsets; the entry points came without a new ABI version, BsvdConvArgs and BsvdYuvDesc
    as they were."""
    from bsvd_amd import _lib
    lib = _lib.load()
    Sf = _lib.BsvdYuvSurface
    assert ctypes.sizeof(Sf) == 88
    got = {n: getattr(Sf, n).offset for n, _ in Sf._fields_}
    assert got == {"subsampling": 0, "layout": 4, "bits": 8, "high_bits": 12, "matrix": 16, "full_range": 20, "chroma": 24, "reserved0": 28,
                   "pitch": 32, "reserved1": 44, "offset": 48, "frame_stride": 72, "reserved2": 80}
    assert _lib.ABI_VERSION == 12 and lib.bsvd_abi_version() == 12
    assert ctypes.sizeof(_lib.BsvdConvArgs) == 272 == lib.bsvd_conv_args_size()
    assert ctypes.sizeof(_lib.BsvdYuvDesc) == 32
    for name in ("bsvd_yuv_frame_bytes", "bsvd_yuv_to_planar", "bsvd_planar_to_yuv", "bsvd_yuv_to_planar_pad", "bsvd_planar_to_yuv_crop"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def _call_all(a, pad):
    """-> [(entry point, rc, error text)] of the decode and the encode entry point, plain or pad / crop"""
    from bsvd_amd import _lib
    lib = _lib.load()
    out = []
    if pad:
        rc = lib.bsvd_yuv_to_planar_pad(a["yuv"], a["planar"], a["frames"], a["H"], a["W"], a["Hp"], a["Wp"], a["surface"], a["cc"], 0.1, None)
        out.append(("bsvd_yuv_to_planar_pad", rc, lib.bsvd_last_error().decode()))
        rc = lib.bsvd_planar_to_yuv_crop(a["planar"], a["yuv"], a["frames"], a["Hp"], a["Wp"], a["H"], a["W"], a["surface"], None)
        out.append(("bsvd_planar_to_yuv_crop", rc, lib.bsvd_last_error().decode()))
    else:
        rc = lib.bsvd_yuv_to_planar(a["yuv"], a["planar"], a["frames"], a["H"], a["W"], a["surface"], a["cc"], 0.1, None)
        out.append(("bsvd_yuv_to_planar", rc, lib.bsvd_last_error().decode()))
        rc = lib.bsvd_planar_to_yuv(a["planar"], a["yuv"], a["frames"], a["H"], a["W"], a["surface"], None)
        out.append(("bsvd_planar_to_yuv", rc, lib.bsvd_last_error().decode()))
    return out


# (format, changes to a valid 8 x 12 call, the words the error must contain): every case of the header's list
BAD = [
    ("yuv420p", dict(yuv=None), "is NULL"),
    ("yuv420p", dict(planar=None), "is NULL"),
    ("yuv420p", dict(surface=None), "surface is NULL"),
    ("uyvy422", dict(frames=0), "frames"),
    ("uyvy422", dict(frames=-1), "frames"),
    ("yuv444p", dict(s=dict(subsampling=3)), "subsampling"),
    ("yuv444p", dict(s=dict(subsampling=-1)), "subsampling"),
    ("yuv444p", dict(s=dict(layout=4)), "layout"),
    ("yuv444p", dict(s=dict(layout=-1)), "layout"),
    ("yuv444p", dict(s=dict(bits=12)), "bits"),
    ("yuv444p", dict(s=dict(bits=0)), "bits"),
    ("yuv444p10le", dict(s=dict(high_bits=2)), "high_bits"),
    ("yuv444p", dict(s=dict(high_bits=1)), "high_bits"),                        # 8 bit has no ignored bits
    ("nv16", dict(s=dict(matrix=3)), "matrix"),
    ("nv16", dict(s=dict(matrix=-1)), "matrix"),
    ("nv16", dict(s=dict(full_range=2)), "full_range"),
    ("nv16", dict(s=dict(chroma=2)), "chroma"),
    ("yuv444p", dict(s=dict(chroma=2)), "chroma"),                              # ignored at 4:4:4, but an enum value all the same
    ("p210le", dict(s=dict(reserved0=1)), "reserved0"),
    ("p210le", dict(s=dict(reserved1=1)), "reserved1"),
    ("p210le", dict(s=dict(reserved2=1)), "reserved2"),
    # the combinations that are not served
    ("yuv420p", dict(s=dict(layout=1)), "layout"),                              # 4:2:0 semi-planar is NV12: bsvd_yuv420_*
    ("yuv420p10le", dict(s=dict(layout=1, high_bits=1)), "layout"),             # ... and P010
    ("yuv420p", dict(s=dict(layout=2)), "layout"),
    ("yuv420p", dict(s=dict(layout=3)), "layout"),
    ("yuv444p", dict(s=dict(layout=1)), "layout"),                              # NV24
    ("yuv444p", dict(s=dict(layout=2)), "layout"),
    ("uyvy422", dict(s=dict(bits=10)), "bits"),
    ("yuyv422", dict(s=dict(bits=10, high_bits=1)), "bits"),
    ("yuv420p10le", dict(s=dict(high_bits=1)), "high_bits"),
    ("yuv422p10le", dict(s=dict(high_bits=1)), "high_bits"),
    ("yuv444p10le", dict(s=dict(high_bits=1)), "high_bits"),
    ("p210le", dict(s=dict(high_bits=0)), "high_bits"),
    # pitches, offsets, stride, alignment
    ("yuv420p", dict(s=dict(pitch=(11, 0, 0))), "pitch[0]"),                    # W = 12 samples
    ("yuv420p", dict(s=dict(pitch=(0, 5, 0))), "pitch[1]"),                     # 6 chroma samples
    ("yuv420p", dict(s=dict(pitch=(0, 0, 5))), "pitch[2]"),
    ("yuv444p", dict(s=dict(pitch=(0, 11, 0))), "pitch[1]"),
    ("uyvy422", dict(s=dict(pitch=(23, 0, 0))), "pitch[0]"),                    # 12 pixels are 24 bytes
    ("nv16", dict(s=dict(pitch=(0, 11, 0))), "pitch[1]"),                       # 6 CbCr pairs are 12 bytes
    ("p210le", dict(s=dict(pitch=(22, 0, 0))), "pitch[0]"),
    ("p210le", dict(s=dict(pitch=(0, 33, 0))), "pitch[1]"),                     # odd with 16-bit samples
    ("yuv422p10le", dict(s=dict(pitch=(0, 0, 13))), "pitch[2]"),
    ("uyvy422", dict(s=dict(pitch=(0, 32, 0))), "pitch[1]"),                    # a plane the layout does not have
    ("nv16", dict(s=dict(pitch=(0, 0, 32))), "pitch[2]"),
    ("yuyv422", dict(s=dict(offset=(0, 64, 0))), "offset[1]"),
    ("nv16", dict(s=dict(offset=(0, 0, 512))), "offset[2]"),
    ("yuv420p", dict(s=dict(offset=(-1, 0, 0))), "offset[0]"),
    ("yuv420p", dict(s=dict(offset=(0, -96, 0))), "offset[1]"),
    ("yuv420p10le", dict(s=dict(offset=(1, 0, 0))), "offset[0]"),               # odd with 16-bit samples
    ("yuv444p10le", dict(s=dict(offset=(0, 0, 1001))), "offset[2]"),
    ("p210le", dict(yuv=4097), "2-byte aligned"),
    ("yuv422p10le", dict(yuv=4097), "2-byte aligned"),
    ("yuv420p", dict(s=dict(frame_stride=143)), "frame_stride"),                # one tight 8 x 12 frame is 144 bytes
    ("yuv444p", dict(s=dict(frame_stride=287)), "frame_stride"),                # ... 288 at 4:4:4
    ("uyvy422", dict(s=dict(pitch=(64, 0, 0), frame_stride=192)), "frame_stride"),
    ("yuv420p", dict(s=dict(offset=(16, 0, 0), frame_stride=144)), "frame_stride"),
    ("yuv420p10le", dict(s=dict(frame_stride=289)), "frame_stride"),            # 16-bit frames an odd number of bytes apart
    ("yuv420p", dict(planar=4100), "16-byte aligned"),
]
BAD_PLAIN = [
    ("yuv420p", dict(H=0), "H = 0"), ("yuv420p", dict(H=-8), "H = -8"), ("yuv422p", dict(H=6), "H = 6"), ("yuv444p", dict(H=7), "H = 7"),
    ("yuv420p", dict(W=0), "W = 0"), ("uyvy422", dict(W=10), "W = 10"), ("yuv444p", dict(W=9), "W = 9"),
]
BAD_PAD = [
    ("yuv420p", dict(H=0), "H = 0"), ("yuv420p", dict(H=7), "H = 7"), ("yuv420p", dict(W=11), "W = 11"), ("yuv420p", dict(W=0), "W = 0"),
    ("yuv422p", dict(H=1, Hp=1), "H = 1"), ("nv16", dict(W=11), "W = 11"), ("uyvy422", dict(W=-2), "W = -2"),
    ("yuv444p", dict(H=1, Hp=1), "H = 1"), ("yuv444p", dict(W=1, Wp=4), "W = 1"), ("yuv444p10le", dict(H=0), "H = 0"),
    ("yuv422p", dict(Hp=7), "Hp = 7"), ("yuv422p", dict(Wp=8), "Wp = 8"),                        # below the picture
    ("yuv444p", dict(H=4, Hp=8), "Hp = 8"), ("yuv444p", dict(W=4, Wp=8), "Wp = 8"),              # a pad of a whole dimension
    ("yuv420p", dict(Hp=9), "Hp = 9"),                                                             # 4:2:0: Hp even
    ("uyvy422", dict(Wp=14), "Wp = 14"), ("yuv444p", dict(W=11, Wp=11), "Wp = 11"),               # float4 rows
]


def _check_refusal(pix_fmt, change, words, pad):
    change = dict(change)
    s = _surface(pix_fmt, **change.pop("s", {}))
    a = dict(yuv=4096, planar=8192, frames=2, H=8, W=12, Hp=8, Wp=12, surface=ctypes.byref(s), cc=1)
    a.update(change)
    for fn, rc, err in _call_all(a, pad):
        assert rc == -3, (fn, rc)
        assert err.startswith(fn + ": ") and words in err, err
        if "NULL" in words and "surface" not in words:
            decode = "to_planar" in fn
            assert (("src" if decode else "dst") if change.get("yuv", 1) is None else ("dst" if decode else "src")) in err, err


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("pix_fmt,change,words", BAD)
def test_validation_names_the_argument(pix_fmt, change, words, pad):
    """All four converting entry points refuse each bad argument with -3 and say which one -- before any launch, without a device."""
    _check_refusal(pix_fmt, change, words, pad)


@pytest.mark.parametrize("pix_fmt,change,words", BAD_PLAIN)
def test_validation_of_the_plain_sizes(pix_fmt, change, words):
    _check_refusal(pix_fmt, change, words, 0)


@pytest.mark.parametrize("pix_fmt,change,words", BAD_PAD)
def test_validation_of_the_pad_and_crop_sizes(pix_fmt, change, words):
    _check_refusal(pix_fmt, change, words, 1)


def test_validation_const_channels():
    from bsvd_amd import _lib
    lib = _lib.load()
    s = _surface("uyvy422")
    assert lib.bsvd_yuv_to_planar(4096, 8192, 1, 8, 12, ctypes.byref(s), -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()
    assert lib.bsvd_yuv_to_planar_pad(4096, 8192, 1, 5, 10, 8, 12, ctypes.byref(s), -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()


def test_the_yuv420_entry_points_still_refuse_other_formats():
    from bsvd_amd import _lib
    lib = _lib.load()
    for pix_fmt in (2, 3, -1):
        d = _lib.BsvdYuvDesc(pix_fmt=pix_fmt, matrix=1, full_range=0, chroma=1)
        assert lib.bsvd_yuv420_to_planar(4096, 8192, 1, 8, 12, ctypes.byref(d), 0, 0.0, None) == -3
        assert "pix_fmt" in lib.bsvd_last_error().decode()
        assert lib.bsvd_yuv420_frame_bytes(8, 12, pix_fmt, 0) == -1


def test_frame_io_argument_errors():
    """Names and host-side checks come before the device is asked for."""
    import torch
    from bsvd_amd.frame_io import output_to_yuv, output_to_yuv420, yuv420_to_input, yuv_to_input
    buf = torch.zeros((1, 288), dtype=torch.uint8)
    for kw in (dict(pix_fmt="yv12"), dict(pix_fmt="nv12"), dict(pix_fmt="yuv444"), dict(pix_fmt="v210"), dict(matrix="bt470"), dict(chroma="cubic"),
               dict(pitches=[8]), dict(pitches=[16, 16, 16, 16]), dict(pix_fmt="uyvy422", pitches=[32, 32]), dict(pitches=[-16]),
               dict(pix_fmt="uyvy422", offsets=[0, 8]), dict(pix_fmt="yuv420p10le", pitches=[25])):
        with pytest.raises(ValueError):
            yuv_to_input(buf, 8, 12, **kw)
    with pytest.raises(ValueError):
        yuv_to_input(buf, 8, 10, "yuv420p")                         # plain: multiples of 4
    with pytest.raises(ValueError):
        yuv_to_input(buf, 7, 10, "yuv420p", pad_to=(8, 12))         # 4:2:0: even
    with pytest.raises(ValueError):
        yuv_to_input(buf, 5, 7, "uyvy422", pad_to=(8, 8))           # 4:2:2: even W
    with pytest.raises(ValueError):
        output_to_yuv(torch.zeros((1, 3, 8, 12)), "yuv422p")        # not on the device
    with pytest.raises(ValueError):
        output_to_yuv(torch.zeros((1, 4, 8, 12)), "yuv422p")
    # the yuv420 pair knows the names it knew
    with pytest.raises(ValueError):
        yuv420_to_input(buf, 8, 12, pix_fmt="yv12")
    with pytest.raises(ValueError):
        yuv420_to_input(buf, 8, 12, pix_fmt="yuv420p")
    with pytest.raises(ValueError):
        output_to_yuv420(torch.zeros((1, 3, 8, 12)), pix_fmt="yuv420p")


def test_pipeline_argument_errors_and_frame_geometry():
    """Names, colour and frame_shape are checked when a pipeline is constructed, before its model or a device is touched; a frame is a 1-D
    array of the tight frame's samples, a clip [T, n]."""
    from bsvd_amd.pipeline import ClipPipeline, Colour, LiveStream, _pixel_format
    for cls in (ClipPipeline, LiveStream):
        for name in ("yuv444", "yv12", "nv21", "v210", "yuv420p12le"):
            with pytest.raises(ValueError, match="pix_fmt"):
                cls(None, pix_fmt=name, frame_shape=(8, 12))
        for name in NAMES:
            with pytest.raises(ValueError, match="frame_shape"):
                cls(None, pix_fmt=name)
            with pytest.raises(ValueError, match="matrix"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), colour={"matrix": "bt470"})
            with pytest.raises(ValueError, match="chroma"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), colour=Colour(chroma="cubic"))
            with pytest.raises(ValueError, match="colour"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), colour={"gamma": 2.2})
            with pytest.raises(ValueError, match="row_pitch"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), colour={"row_pitch": 64})
            with pytest.raises(ValueError, match="width"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), colour={"width": 8})
            with pytest.raises(ValueError):
                cls(None, pix_fmt=name, frame_shape=(6, 10))                           # no pad: multiples of 4
            with pytest.raises(ValueError, match="pad"):
                cls(None, pix_fmt=name, frame_shape=(8, 12), pad="edge")
        with pytest.raises(ValueError):
            cls(None, pix_fmt="yuv420p", frame_shape=(5, 10), pad="reflect")
        with pytest.raises(ValueError):
            cls(None, pix_fmt="uyvy422", frame_shape=(5, 7), pad="reflect")
        with pytest.raises(ValueError):
            cls(None, pix_fmt="yuv444p", frame_shape=(2, 2), pad="reflect")            # a pad of 2 is not below the dimension
    for name in NAMES:
        f = S.FORMATS[name]
        dtype = np.uint16 if f.bits > 8 else np.uint8
        H, W = {420: (6, 10), 422: (5, 10), 444: (5, 7)}[f.sub]
        for pad, (h, w) in ((None, (8, 12)), ("reflect", (H, W))):
            fmt = _pixel_format(name, {"matrix": "bt601"}, pad, (h, w))
            nbytes = S.frame_bytes(h, w, name)
            n = nbytes // np.dtype(dtype).itemsize
            assert fmt.dtype == np.dtype(dtype) and fmt.samples == n
            g = fmt.geometry(np.zeros(n, dtype), clip=False)
            assert (g.h, g.w, g.staging, g.row_pitch, g.net_h, g.net_w) == (h, w, (nbytes,), None, 8, 12 if w > 7 else 8)
            g = fmt.geometry(np.zeros((3, n), dtype), clip=True)
            assert (g.h, g.w, g.staging, g.row_pitch) == (h, w, (3, nbytes), None)
            for frame in (np.zeros(n, np.uint16 if dtype == np.uint8 else np.uint8),   # wrong dtype for the format
                          np.zeros(n + 1, dtype), np.zeros(n - 1, dtype),              # not the tight frame
                          np.zeros((3, n), dtype),                                      # a clip where a frame is expected
                          np.zeros((h, w, 3), np.uint8)):                               # an RGB frame
                with pytest.raises(ValueError):
                    fmt.geometry(frame, clip=False)
            with pytest.raises(ValueError):
                fmt.geometry(np.zeros(n, dtype), clip=True)
