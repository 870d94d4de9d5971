"""Frame I/O for any picture size (bsvd_u8_to_planar_pad / bsvd_planar_to_u8_crop / bsvd_yuv420_to_planar_pad / bsvd_planar_to_yuv420_crop,
frame_io's pad_to / crop_to, pad='reflect' of the pipelines): what needs no device -- the exports and the unchanged ABI, the picture-size
arithmetic, every refusal with its error text, the numpy pad model against denoise.pad_to_multiple_of_4 (the rule golden g8 pins), the
inputs of the GPU encode test against its near-half cap, and the pipelines' geometry."""
import ctypes
import itertools

import numpy as np
import pytest

import yuv_model as M
import yuv_pad_model as P

NEW = ("bsvd_u8_to_planar_pad", "bsvd_planar_to_u8_crop", "bsvd_yuv420_picture_bytes", "bsvd_yuv420_to_planar_pad", "bsvd_planar_to_yuv420_crop")


def test_exports_and_unchanged_abi():
    from bsvd_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 12 and lib.bsvd_abi_version() == 12
    assert ctypes.sizeof(_lib.BsvdConvArgs) == 272 == lib.bsvd_conv_args_size()
    D = _lib.BsvdYuvDesc
    assert ctypes.sizeof(D) == 32 and D.frame_stride.offset == 24 and D.row_pitch.offset == 16 and D.reserved.offset == 20


def test_picture_bytes():
    from bsvd_amd import _lib
    from bsvd_amd.frame_io import network_size, yuv420_picture_bytes
    lib = _lib.load()
    NV12, P010 = _lib.PIX_FMT["nv12"], _lib.PIX_FMT["p010"]
    assert lib.bsvd_yuv420_picture_bytes(480, 854, NV12, 0) == 854 * 480 * 3 // 2
    assert lib.bsvd_yuv420_picture_bytes(480, 854, P010, 0) == 2 * 854 * 480 * 3 // 2
    assert lib.bsvd_yuv420_picture_bytes(30, 42, P010, 192) == 192 * 45
    assert lib.bsvd_yuv420_picture_bytes(6, 10, NV12, 11) == 11 * 9                 # NV12 pitches need no alignment
    assert lib.bsvd_yuv420_picture_bytes(8, 12, NV12, 0) == lib.bsvd_yuv420_frame_bytes(8, 12, NV12, 0)
    for bad in ((7, 10, NV12, 0), (6, 9, NV12, 0), (0, 10, NV12, 0), (6, -2, NV12, 0), (6, 10, 2, 0), (6, 10, NV12, 9), (6, 10, P010, 18),
                (6, 10, P010, 21), (6, 10, NV12, -16)):
        assert lib.bsvd_yuv420_picture_bytes(*bad) == -1, bad
    assert lib.bsvd_yuv420_frame_bytes(8, 10, NV12, 0) == -1                        # the multiple-of-4 entry is what it was
    assert lib.bsvd_yuv420_frame_bytes(6, 8, NV12, 0) == -1
    assert yuv420_picture_bytes(480, 854, "nv12") == 854 * 480 * 3 // 2
    assert yuv420_picture_bytes(30, 42, "p010", 192) == 192 * 45
    for bad in ((6, 10, "yuyv"), (7, 10, "nv12"), (6, 10, "p010", 21)):
        with pytest.raises(ValueError):
            yuv420_picture_bytes(*bad)
    assert network_size(480, 854) == (480, 856) and network_size(30, 50) == (32, 52) and network_size(3, 1) == (4, 4) and network_size(8, 12) == (8, 12)


def _desc(**kw):
    from bsvd_amd import _lib
    return _lib.BsvdYuvDesc(**{"pix_fmt": 0, "matrix": 1, "full_range": 0, "chroma": 1, **kw})


def _yuv_calls(lib, a):
    """the two YUV entry points on the arguments ``a`` -> [(name, rc, error text)]"""
    out = []
    rc = lib.bsvd_yuv420_to_planar_pad(a["yuv"], a["planar"], a["frames"], a["H"], a["W"], a["Hp"], a["Wp"], a["desc"], a.get("cc", 1), 0.1, None)
    out.append(("bsvd_yuv420_to_planar_pad", rc, lib.bsvd_last_error().decode()))
    rc = lib.bsvd_planar_to_yuv420_crop(a["planar"], a["yuv"], a["frames"], a["Hp"], a["Wp"], a["H"], a["W"], a["desc"], None)
    out.append(("bsvd_planar_to_yuv420_crop", rc, lib.bsvd_last_error().decode()))
    return out


# (changes to a valid call -- an 8 x 12 NV12 picture into a 12 x 16 tensor --, the words the error must contain)
YUV_BAD = [
    (dict(Hp=6), "Hp = 6"),                                                     # below H
    (dict(Wp=8), "Wp = 8"),                                                     # below W
    (dict(Hp=16), "Hp = 16"),                                                   # a pad of a whole dimension
    (dict(Hp=18), "Hp = 18"),                                                   # ... or more
    (dict(Wp=24), "Wp = 24"),
    (dict(H=7), "H = 7"),                                                       # odd
    (dict(W=11), "W = 11"),
    (dict(H=0), "H = 0"),
    (dict(W=-2), "W = -2"),
    (dict(Hp=11), "Hp = 11"),                                                   # odd
    (dict(Wp=14), "Wp = 14"),                                                   # not a multiple of 4
    (dict(yuv=None), "is NULL"),
    (dict(planar=None), "is NULL"),
    (dict(desc=None), "desc is NULL"),
    (dict(frames=0), "frames"),
    (dict(d=dict(pix_fmt=2)), "pix_fmt"),
    (dict(d=dict(matrix=3)), "matrix"),
    (dict(d=dict(full_range=2)), "full_range"),
    (dict(d=dict(chroma=2)), "chroma"),
    (dict(d=dict(reserved=1)), "reserved"),
    (dict(d=dict(row_pitch=11)), "row_pitch"),                                  # W = 12 samples
    (dict(d=dict(pix_fmt=1, row_pitch=22)), "row_pitch"),                       # 12 P010 samples are 24 bytes
    (dict(d=dict(pix_fmt=1, row_pitch=33)), "row_pitch"),                       # odd
    (dict(d=dict(pix_fmt=1), yuv=4097), "2-byte aligned"),
    (dict(d=dict(frame_stride=12 * 12 - 1)), "frame_stride"),                   # one tight 8 x 12 NV12 picture is 144 bytes
    (dict(d=dict(row_pitch=64, frame_stride=12 * 12)), "frame_stride"),
    (dict(d=dict(pix_fmt=1, frame_stride=2 * 12 * 12 + 1)), "frame_stride"),
    (dict(planar=4100), "16-byte aligned"),
]


@pytest.mark.parametrize("change,words", YUV_BAD)
def test_yuv_refusals_name_the_argument(change, words):
    """-3 and the argument's name from both entry points, before any launch: the pointers are dummies"""
    from bsvd_amd import _lib
    lib = _lib.load()
    change = dict(change)
    d = _desc(**change.pop("d", {}))
    a = dict(yuv=4096, planar=8192, frames=2, H=8, W=12, Hp=12, Wp=16, desc=ctypes.byref(d))
    a.update(change)
    for name, rc, err in _yuv_calls(lib, a):
        assert rc == -3, (name, rc)
        assert err.startswith(name + ": ") and words in err, err
    assert lib.bsvd_yuv420_to_planar_pad(4096, 8192, 1, 8, 12, 12, 16, ctypes.byref(_desc()), -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()


U8_BAD = [
    (dict(Hp=7), "Hp = 7"), (dict(Wp=11), "Wp = 11"), (dict(Hp=16), "Hp = 16"), (dict(Wp=24), "Wp = 24"), (dict(Wp=30), "Wp = 30"),
    (dict(src=None), "src is NULL"), (dict(dst=None), "dst is NULL"), (dict(frames=0), "frames"), (dict(C=0), "C = 0"), (dict(H=0), "H = 0"),
    (dict(W=-1), "W = -1"),
]


@pytest.mark.parametrize("change,words", U8_BAD)
def test_u8_refusals_name_the_argument(change, words):
    from bsvd_amd import _lib
    lib = _lib.load()
    a = dict(src=4096, dst=8192, frames=2, C=3, H=8, W=12, Hp=12, Wp=16)
    a.update(change)
    rc = lib.bsvd_u8_to_planar_pad(a["src"], a["dst"], a["frames"], a["C"], a["H"], a["W"], a["Hp"], a["Wp"], 1, 1, 0.1, None)
    err = lib.bsvd_last_error().decode()
    assert rc == -3 and err.startswith("bsvd_u8_to_planar_pad: ") and words in err, (rc, err)
    rc = lib.bsvd_planar_to_u8_crop(a["src"], a["dst"], a["frames"], a["C"], a["Hp"], a["Wp"], a["H"], a["W"], 1, 0, None)
    err = lib.bsvd_last_error().decode()
    assert rc == -3 and err.startswith("bsvd_planar_to_u8_crop: ") and words in err, (rc, err)
    assert lib.bsvd_u8_to_planar_pad(4096, 8192, 1, 3, 8, 12, 12, 16, 1, -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()


def test_largest_pad_passes_the_checks():
    """pad = dimension - 1 is the largest pad reflect defines, and the checks accept it.  Asked without a launch: const_channels < 0 is the
    last refusal in line, so it is the one reported exactly when every check on the sizes has passed.  (With 4:2:0 the parities of Hp and
    Wp put the largest legal pad below dimension - 1.)"""
    from bsvd_amd import _lib
    lib = _lib.load()
    assert lib.bsvd_u8_to_planar_pad(4096, 8192, 1, 3, 8, 12, 15, 23, 1, -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()
    assert lib.bsvd_yuv420_to_planar_pad(4096, 8192, 1, 8, 10, 14, 16, ctypes.byref(_desc()), -1, 0.0, None) == -3      # W pad 6 of at most 9, H 6 of 7
    assert "const_channels" in lib.bsvd_last_error().decode()
    assert lib.bsvd_yuv420_to_planar_pad(4096, 8192, 1, 8, 10, 16, 16, ctypes.byref(_desc()), -1, 0.0, None) == -3
    assert "Hp = 16" in lib.bsvd_last_error().decode()


@pytest.mark.parametrize("H,W", [(5, 7), (30, 42), (6, 10)])
def test_pad_model_is_pad_to_multiple_of_4(H, W):
    """The numpy pad the kernels are held to equals the fp32 path's pad (denoise.pad_to_multiple_of_4, pinned by golden g8) bit for bit."""
    import torch
    from bsvd_amd.denoise import pad_to_multiple_of_4
    from bsvd_amd.frame_io import network_size
    x = np.random.RandomState(H * 100 + W).standard_normal((3, 4, H, W)).astype(np.float32)
    want, plist = pad_to_multiple_of_4(torch.from_numpy(x))
    Hp, Wp = network_size(H, W)
    assert plist == [0, Wp - W, 0, Hp - H, 0, 0] and tuple(want.shape[-2:]) == (Hp, Wp)
    got = P.pad_reflect(x, Hp, Wp)
    assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    for m in range(Hp - H):
        assert np.array_equal(got[..., H + m, :], got[..., H - 2 - m, :])
    for m in range(Wp - W):
        assert np.array_equal(got[..., W + m], got[..., W - 2 - m])


@pytest.mark.parametrize("pix_fmt,chroma", list(itertools.product(["nv12", "p010"], ["nearest", "linear"])))
def test_encode_inputs_stay_under_the_near_half_cap(pix_fmt, chroma):
    """tests/test_gpu_frame_pad.py accepts +-1 only where the float64 model's unrounded value is within 1e-3 of a half, and caps such
    samples at 1 % of a case's samples.  The cap is a condition on the seeded inputs: it holds for them, and the float32 model -- the
    arithmetic a conforming kernel does -- satisfies the rule on them."""
    bits = M.BITS[pix_fmt]
    for (H, W), (Hp, Wp) in P.HALF_ITEM_SIZES:
        x = P.rgb(P.T, Hp, Wp)
        vals = P.encode_values_crop(x, H, W, bits, chroma=chroma, dtype=np.float64)
        band = P.near_half(vals)
        near, total = sum(int(b.sum()) for b in band), sum(b.size for b in band)
        assert total == P.T * H * W * 3 // 2
        assert near <= 0.01 * total, (H, W, near, total)
        for v, v32, b in zip(vals, P.encode_values_crop(x, H, W, bits, chroma=chroma, dtype=np.float32), band):
            d = np.rint(v32).astype(np.int64) - np.rint(v).astype(np.int64)
            assert not ((d != 0) & ~(b & (np.abs(d) == 1))).any()


def test_pipeline_geometry_with_reflect_pad():
    from bsvd_amd.pipeline import ClipPipeline, Colour, LiveStream, _pixel_format
    for cls in (ClipPipeline, LiveStream):
        for pix_fmt in ("rgb24", "nv12", "p010"):
            with pytest.raises(ValueError, match="pad"):
                cls(None, pix_fmt=pix_fmt, pad="edge")
    rgb_frame, nv12_frame, p010_clip = np.zeros((30, 50, 3), np.uint8), np.zeros((45, 42), np.uint8), np.zeros((2, 45, 64), np.uint16)
    colour = Colour(row_pitch=128, width=42)
    g = _pixel_format("rgb24", None, pad="reflect").geometry(rgb_frame, clip=False)
    assert (g.h, g.w, g.staging, g.row_pitch, g.net_h, g.net_w) == (30, 50, (30, 50, 3), None, 32, 52)
    g = _pixel_format("rgb24", None, pad="reflect").geometry(np.zeros((3, 5, 7, 3), np.uint8), clip=True)
    assert (g.h, g.w, g.staging, g.net_h, g.net_w) == (5, 7, (3, 5, 7, 3), 8, 8)
    g = _pixel_format("nv12", None, pad="reflect").geometry(nv12_frame, clip=False)
    assert (g.h, g.w, g.staging, g.row_pitch, g.net_h, g.net_w) == (30, 42, (42 * 45,), None, 32, 44)
    g = _pixel_format("p010", colour, pad="reflect").geometry(p010_clip, clip=True)
    assert (g.h, g.w, g.staging, g.row_pitch, g.net_h, g.net_w) == (30, 42, (2, 128 * 45), 128, 32, 44)
    g = _pixel_format("nv12", None, pad="reflect").geometry(np.zeros((96, 96), np.uint8), clip=False)        # a multiple of 4: no pad
    assert (g.h, g.w, g.staging, g.net_h, g.net_w) == (64, 96, (96 * 96,), 64, 96)
    for fmt, frame in ((_pixel_format("nv12", None, pad="reflect"), np.zeros((45, 41), np.uint8)),            # odd W
                       (_pixel_format("nv12", None, pad="reflect"), np.zeros((44, 42), np.uint8)),            # rows are not H * 3 / 2
                       (_pixel_format("nv12", None, pad="reflect"), np.zeros((3, 2), np.uint8)),              # 2 x 2: the pad would be the dimension
                       (_pixel_format("rgb24", None, pad="reflect"), np.zeros((2, 50, 3), np.uint8)),
                       (_pixel_format("rgb24", None, pad="reflect"), np.zeros((30, 50), np.uint8))):
        with pytest.raises(ValueError):
            fmt.geometry(frame, clip=False)
    # pad=None (also when not given): every refusal stays, and the fields the padded geometry adds say "the picture's size"
    for pad in ({}, {"pad": None}):
        for fmt, frame, clip in ((_pixel_format("rgb24", None, **pad), rgb_frame, False), (_pixel_format("nv12", None, **pad), nv12_frame, False),
                                 (_pixel_format("p010", colour, **pad), p010_clip, True)):
            with pytest.raises(ValueError, match="multiples of 4"):
                fmt.geometry(frame, clip=clip)
        g = _pixel_format("rgb24", None, **pad).geometry(np.zeros((64, 96, 3), np.uint8), clip=False)
        assert (g.h, g.w, g.staging, g.row_pitch, g.net_h, g.net_w) == (64, 96, (64, 96, 3), None, 64, 96)


def test_frame_io_pad_arguments_are_checked_before_the_device():
    """without pad_to the old refusal stays (and comes before the device is asked for); a pad_to that is no pair is a ValueError"""
    import torch
    from bsvd_amd.frame_io import yuv420_to_input
    buf = torch.zeros((1, 144), dtype=torch.uint8)
    with pytest.raises(ValueError, match="multiples of 4"):
        yuv420_to_input(buf, 8, 10)
    with pytest.raises(ValueError, match="even"):
        yuv420_to_input(buf, 7, 10, pad_to=(8, 12))
