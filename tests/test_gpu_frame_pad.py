"""Frame I/O for any picture size on the device: frame_io's pad_to / crop_to (bsvd_u8_to_planar_pad / bsvd_planar_to_u8_crop in
tensor_layout.hip, bsvd_yuv420_to_planar_pad / bsvd_planar_to_yuv420_crop in frame_yuv.hip) and pad='reflect' of the pipelines.  References:
the existing entry points + F.pad / a slice wherever they can run (any size for uint8, multiples of 4 for YUV), the numpy model
tests/yuv_pad_model.py for the sizes only the new kernels take.  Sizes are the smallest at which the item map (4 columns, for YUV x 2 rows)
can go wrong: a row shorter than an item, W % 4 of 1, 2 and 3, a half YUV item (W % 4 == 2), an odd number of row pairs, a pad in one
dimension only, both, and none."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yuv_model as M
import yuv_pad_model as P
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = P.T
SIGMA = 30 / 255.0
GUARD = 64          # bytes either side of a frame buffer inside its allocation
U8_SIZES = [((3, 3), (4, 4)), ((5, 7), (8, 8)), ((30, 50), (32, 52)), ((8, 12), (12, 16)), ((8, 12), (8, 12))]
YUV_GRID = list(itertools.product(["nv12", "p010"], ["nearest", "linear"], [False, True]))       # pix_fmt, chroma, pitched


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pad(x, Hp, Wp):
    H, W = x.shape[-2:]
    return F.pad(x, (0, Wp - W, 0, Hp - H), mode="reflect") if (Hp, Wp) != (H, W) else x


# ---- uint8 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", [True, False])
@pytest.mark.parametrize("C", [3, 1])
def test_rgb_in_is_the_reflect_pad_of_the_existing_entry(hwc, C):
    """frames_to_input(pad_to=) == F.pad(frames_to_input(), reflect) as bits; the sigma plane is constant over the whole padded plane."""
    from bsvd_amd.frame_io import frames_to_input
    for ((H, W), (Hp, Wp)), sigma in itertools.product(U8_SIZES, [None, SIGMA]):
        rs = np.random.RandomState(100 * H + W + C)
        x = torch.from_numpy(rs.randint(0, 256, (T, H, W, C) if hwc else (T, C, H, W)).astype(np.uint8)).to(DEV)
        want = _pad(frames_to_input(x, sigma, hwc), Hp, Wp)
        got = frames_to_input(x, sigma, hwc, pad_to=(Hp, Wp))
        assert got.shape == (T, C + (sigma is not None), Hp, Wp) and got.dtype == torch.float32
        assert torch.equal(_bits(got), _bits(want)), (H, W, Hp, Wp, sigma)
        if sigma is not None:
            assert (_bits(got[:, C]) == int(np.float32(sigma).view(np.int32))).all()


def _out_values(C, Hp, Wp):
    """values below 0, above 1, and exact .5 codes (k + 0.5) / 255 among them -- the ties of the round-half-even"""
    rs = np.random.RandomState(10 * Hp + Wp + C)
    y = rs.uniform(-0.2, 1.2, (T, C, Hp, Wp)).astype(np.float32)
    ties = (rs.randint(0, 255, y.shape).astype(np.float32) + np.float32(0.5)) / np.float32(255)
    return np.where(rs.uniform(size=y.shape) < 0.25, ties, y).astype(np.float32)


@pytest.mark.parametrize("hwc", [True, False])
@pytest.mark.parametrize("C", [3, 1])
def test_rgb_out_is_the_existing_entry_on_the_slice(hwc, C):
    """output_to_frames(crop_to=) == output_to_frames(y[..., :H, :W]); pad rows and columns of y (NaN here) reach nothing.  The entry point
    writes into the middle of a larger 0xA5 buffer whose guards stay."""
    import ctypes
    from bsvd_amd import _lib
    from bsvd_amd.frame_io import output_to_frames
    lib = _lib.load()
    for ((H, W), (Hp, Wp)), rgb2bgr in itertools.product(U8_SIZES, [False, True]):
        y = torch.from_numpy(_out_values(C, Hp, Wp)).to(DEV)
        want = output_to_frames(y[..., :H, :W].contiguous(), hwc, rgb2bgr)
        got = output_to_frames(y, hwc, rgb2bgr, crop_to=(H, W))
        assert got.shape == want.shape and got.dtype == torch.uint8
        assert torch.equal(got, want), (H, W, Hp, Wp, rgb2bgr)
        y2 = y.clone()
        y2[..., H:, :] = float("nan")
        y2[..., :, W:] = float("nan")
        assert torch.equal(output_to_frames(y2, hwc, rgb2bgr, crop_to=(H, W)), want)
        n = T * C * H * W
        big = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.bsvd_planar_to_u8_crop(y.data_ptr(), big.data_ptr() + GUARD, T, C, Hp, Wp, H, W, 1 if hwc else 0, 1 if rgb2bgr else 0,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert torch.equal(big[GUARD:GUARD + n], want.reshape(-1)) and (big[:GUARD] == 0xA5).all() and (big[-GUARD:] == 0xA5).all()


# ---- YUV 4:2:0 ------------------------------------------------------------------------------------------------------------------------------
def _layout(H, W, pix_fmt, pitched):
    """(row_pitch, frame_stride) in bytes: tight, or rows rounded up to 64 bytes plus 64 with frames one frame plus 128 apart"""
    if not pitched:
        return None, None
    pitch = (W * (2 if pix_fmt == "p010" else 1) + 63) // 64 * 64 + 64
    return pitch, pitch * H * 3 // 2 + 128


def _surface(buf, fill):
    """host surface [T, stride] -> (whole allocation, device view of the same bytes inside it), GUARD bytes of ``fill`` either side"""
    n, stride = buf.shape
    big = torch.full((GUARD + n * stride + GUARD,), fill, dtype=torch.uint8, device=DEV)
    view = big[GUARD:GUARD + n * stride].view(n, stride)
    view.copy_(torch.from_numpy(buf))
    return big, view


def _decode(H, W, pix_fmt, chroma, pitched, fill, pad_to, sigma=SIGMA):
    from bsvd_amd.frame_io import yuv420_to_input
    Y, Cb, Cr, low = P.codes(pix_fmt, T, H, W)
    pitch, stride = _layout(H, W, pix_fmt, pitched)
    _, view = _surface(M.pack(Y, Cb, Cr, pix_fmt, pitch, stride, fill=fill, low_bits=low), fill)
    return yuv420_to_input(view, H, W, pix_fmt, chroma=chroma, sigma=sigma, row_pitch=pitch, pad_to=pad_to)


@pytest.mark.parametrize("pix_fmt,chroma,pitched", YUV_GRID)
def test_yuv_in_multiples_of_4_match_the_existing_entry(pix_fmt, chroma, pitched):
    """Where the existing entry can run: bit-equal to F.pad of it, and to it when there is nothing to pad."""
    for (H, W), (Hp, Wp) in [((8, 12), (12, 16)), ((36, 52), (36, 52)), ((8, 12), (8, 12))]:
        base = _decode(H, W, pix_fmt, chroma, pitched, 0xFF, None)
        got = _decode(H, W, pix_fmt, chroma, pitched, 0xFF, (Hp, Wp))
        assert got.shape == (T, 4, Hp, Wp)
        assert torch.equal(_bits(got), _bits(_pad(base, Hp, Wp))), (H, W, Hp, Wp)


@pytest.mark.parametrize("pix_fmt,chroma,pitched", YUV_GRID)
def test_yuv_in_half_items_match_the_model_and_mirror_themselves(pix_fmt, chroma, pitched):
    """W % 4 == 2 and odd row-pair counts.  Picture region: max-abs <= 1e-6 against the float64 model, the bound of
    test_gpu_yuv.py::test_decode_matches_the_float64_model (the float32 model is 1.4e-7 from it; a conforming kernel may associate its
    FMAs differently).  Pad region: the bits of its mirror source in the same output.  Bytes that are no sample -- pitch padding, gaps,
    guards -- change from 0x00 to 0xFF without a bit of the result changing; junk in the low 6 bits of P010 words is ignored (the model
    never sees it)."""
    bits = M.BITS[pix_fmt]
    worst = 0.0
    for (H, W), (Hp, Wp) in P.HALF_ITEM_SIZES:
        Y, Cb, Cr, _ = P.codes(pix_fmt, T, H, W)
        want = M.decode(Y, Cb, Cr, bits, chroma=chroma, dtype=np.float64)
        got = _decode(H, W, pix_fmt, chroma, pitched, 0xFF, (Hp, Wp))
        assert got.shape == (T, 4, Hp, Wp) and got.dtype == torch.float32
        g = got.cpu().numpy()
        err = float(np.abs(g[:, :3, :H, :W].astype(np.float64) - want).max())
        worst = max(worst, err)
        print("yuv in %s %s pitched=%s %dx%d->%dx%d: max-abs vs float64 model %.3e" % (pix_fmt, chroma, pitched, H, W, Hp, Wp, err))
        assert err <= 1e-6, (H, W, err)
        u = g.view(np.uint32)
        for m in range(Hp - H):
            assert np.array_equal(u[..., H + m, :], u[..., H - 2 - m, :]), (H, W, "row", m)
        for m in range(Wp - W):
            assert np.array_equal(u[..., W + m], u[..., W - 2 - m]), (H, W, "column", m)
        assert (u[:, 3] == np.float32(SIGMA).view(np.uint32)).all()
        assert torch.equal(_bits(_decode(H, W, pix_fmt, chroma, pitched, 0x00, (Hp, Wp))), _bits(got)), (H, W)
        # against the model's own pad, to the same bound: the mirror is the model's mirror
        assert np.abs(g[:, :3].astype(np.float64) - P.pad_reflect(want, Hp, Wp)).max() <= 1e-6
    assert worst <= 1e-6


def _encode(y, H, W, pix_fmt, chroma, pitched):
    """-> (surface [T, stride] as numpy, the whole allocation) after an encode into memory prefilled with 0xA5"""
    from bsvd_amd.frame_io import output_to_yuv420
    pitch, stride = _layout(H, W, pix_fmt, pitched)
    stride = stride or M.frame_bytes(H, W, pix_fmt)
    big, view = _surface(np.full((T, stride), 0xA5, np.uint8), 0xA5)
    got = output_to_yuv420(y, pix_fmt, chroma=chroma, row_pitch=pitch, out=view, crop_to=(H, W))
    assert got.data_ptr() == view.data_ptr()
    return view.cpu().numpy(), big.cpu().numpy()


@pytest.mark.parametrize("pix_fmt,chroma,pitched", YUV_GRID)
def test_yuv_out_multiple_of_4_matches_the_existing_entry(pix_fmt, chroma, pitched):
    from bsvd_amd.frame_io import output_to_yuv420
    (Hp, Wp), (H, W) = (12, 16), (8, 12)
    y = torch.tensor(P.rgb(T, Hp, Wp)).to(DEV)
    pitch, _ = _layout(H, W, pix_fmt, pitched)
    want = output_to_yuv420(y[..., :H, :W].contiguous(), pix_fmt, chroma=chroma, row_pitch=pitch).cpu().numpy()
    surf, _ = _encode(y, H, W, pix_fmt, chroma, pitched)
    mask = M.sample_mask(T, H, W, pix_fmt, *_layout(H, W, pix_fmt, pitched))
    assert np.array_equal(surf[mask], want[M.sample_mask(T, H, W, pix_fmt, pitch)])
    assert (surf[~mask] == 0xA5).all()


@pytest.mark.parametrize("pix_fmt,chroma,pitched", YUV_GRID)
def test_yuv_out_half_items_match_the_model(pix_fmt, chroma, pitched):
    """The rule of test_gpu_yuv.py::test_encode_matches_the_float64_model per case: codes equal rint of the float64 model of the SLICE except,
    by +-1, where its unrounded value is within 1e-3 of a half; such samples are at most 1 % of the case's samples (a condition on the seeded
    inputs, met by them: tests/test_frame_pad_cpu.py).  Pitch padding, the bytes between frames and 64 bytes either side of the buffer keep
    their 0xA5; P010 low bits are zero; NaN in the pad rows and columns of y changes no byte."""
    bits = M.BITS[pix_fmt]
    for (H, W), (Hp, Wp) in P.HALF_ITEM_SIZES:
        x = P.rgb(T, Hp, Wp)
        vals = P.encode_values_crop(x, H, W, bits, chroma=chroma, dtype=np.float64)
        band = P.near_half(vals)
        near, total = sum(int(b.sum()) for b in band), sum(b.size for b in band)
        print("yuv out %s %s pitched=%s %dx%d<-%dx%d: %d of %d samples within 1e-3 of a half" % (pix_fmt, chroma, pitched, H, W, Hp, Wp, near, total))
        assert near <= 0.01 * total
        y = torch.tensor(x).to(DEV)
        surf, big = _encode(y, H, W, pix_fmt, chroma, pitched)
        pitch, stride = _layout(H, W, pix_fmt, pitched)
        planes = M.unpack(surf, H, W, pix_fmt, pitch)
        for name, got, v, b in zip("Y Cb Cr".split(), planes, vals, band):
            d = got - np.rint(v).astype(np.int64)
            bad = (d != 0) & ~(b & (np.abs(d) == 1))
            assert not bad.any(), (H, W, name, int(bad.sum()), got[bad][:4], v[bad][:4])
        if pix_fmt == "p010":
            assert (planes[3] & 63 == 0).all()
        mask = M.sample_mask(T, H, W, pix_fmt, pitch, stride)
        assert (surf[~mask] == 0xA5).all(), (H, W)
        assert (big[:GUARD] == 0xA5).all() and (big[-GUARD:] == 0xA5).all(), (H, W)
        y2 = y.clone()
        y2[..., H:, :] = float("nan")
        y2[..., :, W:] = float("nan")
        surf2, _ = _encode(y2, H, W, pix_fmt, chroma, pitched)
        assert np.array_equal(surf2, surf), (H, W)


def test_output_to_yuv420_crop_without_out():
    from bsvd_amd.frame_io import output_to_yuv420, yuv420_picture_bytes
    y = torch.tensor(P.rgb(T, 32, 44)).to(DEV)
    for pix_fmt, pitch in (("nv12", None), ("p010", 192)):
        got = output_to_yuv420(y, pix_fmt, row_pitch=pitch, crop_to=(30, 42))
        assert got.shape == (T, yuv420_picture_bytes(30, 42, pix_fmt, pitch)) and got.dtype == torch.uint8
        got = got.cpu().numpy()
        tight, _ = _encode(y, 30, 42, pix_fmt, "linear", False)
        mask = M.sample_mask(T, 30, 42, pix_fmt, pitch)
        assert np.array_equal(got[mask], tight.reshape(-1)) and (got[~mask] == 0).all()       # the result's own padding is zero
    with pytest.raises(ValueError):
        output_to_yuv420(y, crop_to=(34, 42))                        # larger than y
    with pytest.raises(ValueError):
        output_to_yuv420(y, crop_to=(30, 41))


# ---- the pipelines (the small model of tests/test_gpu_yuv.py) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import bsvd_amd
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 11)
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64,
                      pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


def _feed_all(live, frames):
    """-> (results in order, flush included; the per-feed pattern of None / frame)"""
    got, pattern = [], []
    for f in frames:
        r = live.feed(f)
        pattern.append(r is not None)
        if r is not None:
            got.append(r)
    return got + live.flush(), pattern


PH, PW = 30, 42


@pytest.mark.parametrize("depth", [1, 2])
def test_live_stream_rgb_reflect_is_the_host_padded_stream(model, depth):
    """LiveStream(pad='reflect') on 30 x 42 RGB frames == the existing LiveStream fed the same frames reflect-padded on the host as uint8,
    its results cropped (for packed RGB the pad commutes with the conversion): same bytes, same latency, same pattern of None."""
    from bsvd_amd.pipeline import LiveStream
    rs = np.random.RandomState(41)
    frames = rs.randint(0, 256, (20, PH, PW, 3)).astype(np.uint8)
    padded = np.pad(frames, ((0, 0), (0, 2), (0, 2), (0, 0)), mode="reflect")
    ref = LiveStream(model, sigma=SIGMA, depth=depth)
    want, want_pattern = _feed_all(ref, padded)
    live = LiveStream(model, sigma=SIGMA, depth=depth, pad="reflect")
    assert live.latency == ref.latency
    got, pattern = _feed_all(live, frames)
    assert pattern == want_pattern and len(got) == len(want) == 20
    assert all(g.shape == (PH, PW, 3) and g.dtype == np.uint8 for g in got)
    assert np.array_equal(np.stack(got), np.stack(want)[:, :PH, :PW])
    if depth >= 2:                                     # a frame-size change with a step in flight still raises (depth 1 has none in flight)
        assert live.feed(frames[0]) is None
        with pytest.raises(ValueError, match="mid-stream"):
            live.feed(frames[0][:, :40])
        live.flush()
    with pytest.raises(ValueError, match="multiples of 4"):
        LiveStream(model, sigma=SIGMA, depth=depth).feed(np.zeros((30, 50, 3), np.uint8))


def _direct_yuv(m, frames, H, W, pix_fmt, row_pitch=None):
    """the synchronous path on the same surfaces: [T, H*3/2, pitch] array -> array"""
    from bsvd_amd.frame_io import network_size, output_to_yuv420, yuv420_to_input
    dev = torch.from_numpy(frames.view(np.uint8).reshape(frames.shape[0], -1)).to(DEV)
    y = m.clip_forward(yuv420_to_input(dev, H, W, pix_fmt, sigma=SIGMA, row_pitch=row_pitch, pad_to=network_size(H, W)))
    return output_to_yuv420(y, pix_fmt, row_pitch=row_pitch, crop_to=(H, W)).cpu().numpy().view(frames.dtype).reshape(frames.shape)


@pytest.mark.parametrize("pix_fmt,pitched", [("nv12", False), ("p010", True)])
def test_live_stream_yuv_reflect_is_the_direct_path(model, pix_fmt, pitched):
    from bsvd_amd.pipeline import LiveStream
    dtype, top = (np.uint8, 256) if pix_fmt == "nv12" else (np.uint16, 65536)
    pitch = 64 if pitched else PW                                    # samples
    colour = {"row_pitch": pitch * np.dtype(dtype).itemsize, "width": PW} if pitched else None
    frames = np.random.RandomState(43).randint(0, top, (20, PH * 3 // 2, pitch)).astype(dtype)
    want = _direct_yuv(model, frames, PH, PW, pix_fmt, colour["row_pitch"] if pitched else None)
    live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt=pix_fmt, colour=colour, pad="reflect", frame_shape=(PH, PW))
    assert live.latency_final
    got, pattern = _feed_all(live, frames)
    assert pattern.index(True) == live.latency
    assert len(got) == 20 and all(g.dtype == dtype and g.shape == frames.shape[1:] for g in got)
    assert np.array_equal(np.stack(got), want)


def test_clip_pipeline_reflect_matches_the_direct_paths(model):
    from bsvd_amd.frame_io import frames_to_input, network_size, output_to_frames
    from bsvd_amd.pipeline import ClipPipeline
    rs = np.random.RandomState(47)
    clip = rs.randint(0, 256, (4, PH, PW, 3)).astype(np.uint8)
    x = frames_to_input(torch.from_numpy(clip).to(DEV), SIGMA, pad_to=network_size(PH, PW))
    want = output_to_frames(model.clip_forward(x), crop_to=(PH, PW)).cpu().numpy()
    (got,) = list(ClipPipeline(model, sigma=SIGMA, depth=2, pad="reflect").run([clip]))
    assert got.shape == clip.shape and got.dtype == np.uint8 and np.array_equal(got, want)
    surf = rs.randint(0, 256, (4, PH * 3 // 2, PW)).astype(np.uint8)
    (got,) = list(ClipPipeline(model, sigma=SIGMA, depth=2, pix_fmt="nv12", pad="reflect").run([surf]))
    assert got.shape == surf.shape and got.dtype == np.uint8 and np.array_equal(got, _direct_yuv(model, surf, PH, PW, "nv12"))
    with pytest.raises(ValueError, match="multiples of 4"):
        ClipPipeline(model, sigma=SIGMA).submit(np.zeros((2, 30, 50, 3), np.uint8))


def test_reflect_on_a_multiple_of_4_is_the_unpadded_pipeline(model):
    from bsvd_amd.pipeline import ClipPipeline
    rs = np.random.RandomState(53)
    clip = rs.randint(0, 256, (4, 32, 48, 3)).astype(np.uint8)
    (a,) = list(ClipPipeline(model, sigma=SIGMA, depth=1).run([clip]))
    (b,) = list(ClipPipeline(model, sigma=SIGMA, depth=1, pad="reflect").run([clip]))
    assert np.array_equal(a, b)
    surf = rs.randint(0, 256, (4, 48, 48)).astype(np.uint8)
    (a,) = list(ClipPipeline(model, sigma=SIGMA, depth=1, pix_fmt="nv12").run([surf]))
    (b,) = list(ClipPipeline(model, sigma=SIGMA, depth=1, pix_fmt="nv12", pad="reflect").run([surf]))
    assert np.array_equal(a, b)
