"""RGB surfaces on the device (bsvd_amd/csrc/frame_rgb.hip: bsvd_rgb_to_planar / bsvd_planar_to_rgb, through ctypes and through
frame_io.rgb_to_input / output_to_rgb and the pipelines' pix_fmt): every name of _lib.RGB_FORMATS, both directions, bit for bit against
the numpy model tests/rgb_surface_model.py, and the memory contract.

Shapes are the smallest at which a path changes.  H = 4 with W in 4, 12, 20, 36, 52: one whole item, an odd item count, rows of items
over one and several waves' worth of lanes.  5 x 7 -> 8 x 8 and 6 x 10 -> 8 x 12: rows that end in part items of 3 and 2 pixels, mirror
rows and columns; 5 x 7 -> 9 x 9: Wp % 4 != 0, the scalar fp32 side, and a pad of H - 1 rows, the largest reflect defines.  T = 2 throughout; every shape also runs pitched, with plane offsets and gaps, frames a
frame and 128 bytes apart; 4 x 12 and 5 x 7 with the surface pointer 1, 2, 3 bytes (2 with 16-bit samples, 4 with the x2 words) and the
fp32 tensor 4 bytes off a 16-byte boundary.  Everything lives in poisoned memory: surfaces inside 0xFF (decode: NaN to any float reader) or
0xA5 / 0x5A (encode), the fp32 tensors and alpha planes in the arenas of tests/arena.py."""
import functools

import numpy as np
import pytest
import torch

import arena
import rgb_surface_model as R
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

T = 2
NAMES = sorted(R.FORMATS)
PLAIN = [(4, 4), (4, 12), (4, 20), (4, 36), (4, 52)]
PADDED = [((5, 7), (8, 8)), ((6, 10), (8, 12)), ((5, 7), (9, 9))]
SHAPES = [(s, s) for s in PLAIN] + PADDED
GUARD = 64          # bytes in front of a surface inside its allocation (the allocation is 256-byte aligned, so is the surface at shift 0)
SIGMA = 30 / 255.0
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _layouts(H, W, name):
    """(pitches, offsets, frame_stride): tight; and rows rounded up to 64 bytes plus 64 and a bit, plane 0 68 bytes into the frame, gaps
    of 36, 20 and 12 bytes behind the planes, frames one frame plus 128 bytes apart"""
    pl = R.planes(H, W, name)
    pitches = [(rb + 63) // 64 * 64 + 64 + 4 * i for i, (_, rb) in enumerate(pl)]
    offsets, at = [], 68
    for i, (rows, _) in enumerate(pl):
        offsets.append(at)
        at += pitches[i] * rows + (36, 20, 12, 0)[i]
    return [(None, None, None), (pitches, offsets, R.frame_bytes(H, W, name, pitches, offsets) + 128)]


def _shifts(name):
    return {1: (1, 2, 3), 2: (2,), 4: (4,)}[R.sample_bytes(name)]


@functools.lru_cache(maxsize=None)
def _codes(bits, H, W):
    """seeded random codes over the full code range, R, G, B and a fourth; shared, never written"""
    rs = np.random.RandomState(100 * H + W + bits)
    out = tuple(rs.randint(0, 1 << bits, (T, H, W)).astype(np.int64) for _ in range(4))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _values(Hp, Wp):
    """seeded uniform(-0.2, 1.2) with exact 0, 1, NaN-free halves sprinkled in: values beyond both clamps and rounding ties; shared"""
    rs = np.random.RandomState(3 * Hp + Wp)
    x = rs.uniform(-0.2, 1.2, (T, 3, Hp, Wp))
    x = np.where(rs.uniform(size=x.shape) < 0.1, rs.randint(0, 511, x.shape) / 510.0, x).astype(np.float32)      # k / 510: ties at 8 bits
    x.setflags(write=False)
    return x


def _surface(name, full_range, pitches, offsets, stride):
    from bsvd_amd import _lib
    layout, components, bits, pos, fourth = _lib.RGB_FORMATS[name]
    s = _lib.BsvdRgbSurface(layout=layout, components=components, bits=bits, fourth=fourth, full_range=1 if full_range else 0)
    s.pos[:] = pos
    s.pitch[:] = tuple(pitches or ()) + (0,) * (4 - len(pitches or ()))
    s.offset[:] = tuple(offsets or ()) + (0,) * (4 - len(offsets or ()))
    s.frame_stride = stride or 0
    return s


def _on_device(buf, fill, shift=0):
    """host bytes [T, stride] -> (the whole allocation, the device pointer of the bytes): GUARD + shift into memory filled with ``fill``"""
    n = buf.size
    big = torch.full((GUARD + shift + n + GUARD,), fill, dtype=torch.uint8, device=DEV)
    big[GUARD + shift:GUARD + shift + n].copy_(torch.from_numpy(buf.reshape(-1)))
    assert big.data_ptr() % 16 == 0
    return big, big.data_ptr() + GUARD + shift


def _fp32_arena(shape, fill, off=0):
    """a tight [T,C,Hp,Wp] tensor between guards; off = 1: four bytes off the 16-byte boundary"""
    a = arena.reserve(shape, 0, fill=fill, device=DEV)
    if off:
        a = arena.Arena(a.size, a.stride, a.offset + off, a.buf.numel() // 4, fill, DEV)
    return a


def _lib_decode(buf, pic, net, name, full_range, layout, shift=0, off=0, const=SIGMA):
    """bsvd_rgb_to_planar on a poisoned surface into 0x00- and 0xFF-filled arenas -> (x, alpha) after the memory checks"""
    import ctypes
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    (H, W), (Hp, Wp) = pic, net
    big, ptr = _on_device(buf, 0xFF, shift)
    before = big.clone()
    s = _surface(name, full_range, *layout)
    sb = min(R.sample_bytes(name), 2)
    runs, alphas = [], []
    for fill in (0x00, 0xFF):
        x = _fp32_arena((T, 3 + (const is not None), Hp, Wp), fill, off)
        al = arena.reserve((T, H, W * sb), 0, fill=fill, device=DEV, dtype=torch.uint8) if R.has_alpha(name) else None
        _lib.check(lib.bsvd_rgb_to_planar(ptr, x.ptr, T, H, W, Hp, Wp, ctypes.byref(s), None if al is None else al.ptr,
                                          0 if const is None else 1, const or 0.0, None), "bsvd_rgb_to_planar")
        torch.cuda.synchronize()
        runs.append(x)
        alphas.append(al)
    assert torch.equal(big, before), "the decode wrote into its surface"
    assert all(r.slack_intact() for r in runs), runs[0].slack_damage()
    assert arena.same_bits(runs[0].logical(), runs[1].logical()), "an element of the tensor was not written"
    alpha = None
    if alphas[0] is not None:
        assert all(a.slack_intact() for a in alphas) and torch.equal(alphas[0].logical(), alphas[1].logical())
        alpha = alphas[0].logical().cpu().numpy().reshape(T, H, -1).view(R.container(name)).reshape(T, H, W)
    return runs[0].logical().cpu().numpy(), alpha


def _lib_encode(y, pic, name, full_range, layout, shift=0, off=0, alpha=None):
    """bsvd_planar_to_rgb from a tensor between NaN guards into surfaces prefilled with 0xA5 and with 0x5A -> the two allocations whole,
    GUARD + shift + T * stride + GUARD bytes"""
    import ctypes
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    H, W = pic
    Hp, Wp = y.shape[-2:]
    src = _fp32_arena(y.shape, 0xFF, off).write(torch.from_numpy(np.array(y)))
    stride = layout[2] or R.frame_bytes(H, W, name)
    s = _surface(name, full_range, *layout)
    al = None
    if alpha is not None:
        al = arena.reserve((T, H, W * alpha.dtype.itemsize), 0, fill=0xFF, device=DEV, dtype=torch.uint8)
        al.write(torch.from_numpy(np.ascontiguousarray(alpha).view(np.uint8).reshape(T, H, -1)))
    out = []
    for fill in (0xA5, 0x5A):
        big, ptr = _on_device(np.full((T, stride), fill, np.uint8), fill, shift)
        _lib.check(lib.bsvd_planar_to_rgb(src.ptr, ptr, T, Hp, Wp, H, W, ctypes.byref(s), None if al is None else al.ptr, None), "bsvd_planar_to_rgb")
        torch.cuda.synchronize()
        out.append(big.cpu().numpy())
    assert src.slack_intact() and arena.same_bits(src.logical(), torch.from_numpy(np.array(y)).to(DEV))
    return out


def _framed(buf, fill, shift):
    return np.concatenate([np.full(GUARD + shift, fill, np.uint8), buf.reshape(-1), np.full(GUARD, fill, np.uint8)])


# ---- against the model, in poisoned memory ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_decode_is_the_model_bit_for_bit(name):
    """both ranges; tight and pitched with offsets, gaps and a frame stride; every byte that is no sample 0xFF, every ignored bit a one; the
    tensor and the alpha plane between guards, every element written, nothing else"""
    f = R.FORMATS[name]
    for pic, net in SHAPES:
        H, W = pic
        r, g, b, fourth = _codes(f.bits, H, W)
        for full_range in (True, False):
            for layout in _layouts(H, W, name):
                buf = R.pack(r, g, b, name, fourth, *layout, fill=0xFF, junk="ones")
                want, want_alpha = R.to_input(buf, H, W, name, full_range, layout[0], layout[1], pad_to=net, const=np.float32(SIGMA))
                got, alpha = _lib_decode(buf, pic, net, name, full_range, layout)
                assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want)), (pic, net, full_range, layout)
                assert (alpha is None) == (want_alpha is None)
                if alpha is not None:
                    assert alpha.dtype == want_alpha.dtype and np.array_equal(alpha, fourth) and np.array_equal(alpha, want_alpha)
    for pic, net in (((4, 12), (4, 12)), ((5, 7), (8, 8))):                   # surface and tensor off their vector alignment
        H, W = pic
        r, g, b, fourth = _codes(f.bits, H, W)
        buf = R.pack(r, g, b, name, fourth, fill=0xFF, junk="ones")
        want, _ = R.to_input(buf, H, W, name, True, pad_to=net, const=np.float32(SIGMA))
        for shift in _shifts(name):
            got, alpha = _lib_decode(buf, pic, net, name, True, (None, None, None), shift=shift, off=shift & 1)
            assert np.array_equal(_bits(got), _bits(want)), (pic, net, shift)
            assert alpha is None or np.array_equal(alpha, fourth)
        got, _ = _lib_decode(buf, pic, net, name, True, (None, None, None), off=1)
        assert np.array_equal(_bits(got), _bits(want)), (pic, net, "tensor + 4 bytes")


@pytest.mark.parametrize("name", NAMES)
def test_encode_is_the_model_bit_for_bit(name):
    """the whole allocation, guards, pitch padding, gaps and all, equals the model's surface laid into the same prefill -- for two prefills,
    so every sample was written and no other byte; pad rows and columns of the tensor hold NaN and reach nothing; alpha codes come from the
    side plane, masked to the format's bits; without it, and for a filler, the maximum code"""
    f = R.FORMATS[name]
    for pic, net in SHAPES:
        H, W = pic
        y = _values(*net).copy()
        y[:, :, H:, :] = np.nan
        y[:, :, :, W:] = np.nan
        alpha = None
        if R.has_alpha(name):
            alpha = np.random.RandomState(H + W).randint(0, 1 << 16, (T, H, W)).astype(R.container(name))     # bits above `bits` set: masked
        for full_range in (True, False):
            for layout in _layouts(H, W, name):
                for a in ((alpha, None) if alpha is not None and full_range else (alpha,)):
                    got = _lib_encode(y, pic, name, full_range, layout, alpha=a)
                    for big, fill in zip(got, (0xA5, 0x5A)):
                        want = R.to_surface(y, name, full_range, *layout, crop_to=pic, alpha=a, fill=fill)
                        assert np.array_equal(big, _framed(want, fill, 0)), (pic, net, full_range, layout, a is None, fill)
    for pic, net in (((4, 12), (4, 12)), ((5, 7), (8, 8))):
        H, W = pic
        y = _values(*net)
        for shift in _shifts(name):
            for big, fill in zip(_lib_encode(y, pic, name, True, (None, None, None), shift=shift, off=shift & 1), (0xA5, 0x5A)):
                assert np.array_equal(big, _framed(R.to_surface(y, name, crop_to=pic, fill=fill), fill, shift)), (pic, shift, fill)
    if f.layout == "x2":
        assert R.unpack(R.to_surface(_values(4, 4), name), 4, 4, name)[4] == 3


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_returns_every_code(name):
    """decode then encode on the device: every code of the format's range at full range (all 65536 at 16 bits), the legal codes at limited
    range and the nearest legal end for the others; alpha through the side plane; a filler comes back as all ones"""
    from bsvd_amd.frame_io import output_to_rgb, rgb_to_input
    f = R.FORMATS[name]
    n = 1 << f.bits
    H, W = 4, n // 4 if n <= 4096 else 256
    Tn = n // (H * W)
    ramp = np.arange(n, dtype=np.int64).reshape(Tn, H, W)
    fourth = ramp[::-1, ::-1, ::-1]
    buf = torch.from_numpy(R.pack(ramp, (ramp + 1) % n, n - 1 - ramp, name, fourth)).to(DEV)
    for full_range in (True, False):
        if R.has_alpha(name):
            x, alpha = rgb_to_input(buf, H, W, name, full_range=full_range, return_alpha=True)
            back = output_to_rgb(x, name, full_range=full_range, alpha=alpha)
        else:
            back = output_to_rgb(rgb_to_input(buf, H, W, name, full_range=full_range), name, full_range=full_range)
        r, g, b, four, ignored = R.unpack(back.cpu().numpy(), H, W, name)
        lo, hi = (0, n - 1) if full_range else (16 * (n >> 8), 235 * (n >> 8))
        assert np.array_equal(r, np.clip(ramp, lo, hi)) and np.array_equal(g, np.clip((ramp + 1) % n, lo, hi)) and np.array_equal(b, np.clip(n - 1 - ramp, lo, hi))
        assert ignored == (3 if f.layout == "x2" else 0)
        if R.has_alpha(name):
            assert np.array_equal(four, fourth)
        elif R.has_filler(name):
            assert set(four.ravel()) == {n - 1}


# ---- against the uint8 kernels and among themselves --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pic,net", [((4, 12), None), ((36, 52), None), ((5, 7), (8, 8)), ((6, 10), (8, 12))])
def test_rgb24_and_bgr24_are_the_uint8_kernels_byte_for_byte(pic, net):
    from bsvd_amd.frame_io import frames_to_input, output_to_frames, output_to_rgb, rgb_to_input
    H, W = pic
    px = torch.from_numpy(np.random.RandomState(H * W).randint(0, 256, (T, H, W, 3)).astype(np.uint8)).to(DEV)
    want = frames_to_input(px, SIGMA, pad_to=net)
    assert arena.same_bits(rgb_to_input(px.reshape(T, -1), H, W, "rgb24", sigma=SIGMA, pad_to=net), want)
    assert arena.same_bits(rgb_to_input(px.flip(-1).contiguous().reshape(T, -1), H, W, "bgr24", sigma=SIGMA, pad_to=net), want)
    y = torch.tensor(_values(*(net or pic))).to(DEV)
    crop = pic if net else None
    for name, bgr in (("rgb24", False), ("bgr24", True)):
        assert torch.equal(output_to_rgb(y, name, crop_to=crop).reshape(T, H, W, 3), output_to_frames(y, rgb2bgr=bgr, crop_to=crop)), name


def test_same_samples_same_bits_in_every_layout():
    """8 bits: gbrp, bgra, 0rgb ... decode to the tensor rgb24 gives and encode to its codes; 16 bits: gbrp16le, bgra64le against rgb48le;
    10 bits: x2rgb10le, x2bgr10le against gbrp10le"""
    from bsvd_amd.frame_io import output_to_rgb, rgb_to_input
    groups = [[n for n in NAMES if R.FORMATS[n].bits == 8], [n for n in NAMES if R.FORMATS[n].bits == 16], ["gbrp10le", "gbrap10le", "x2rgb10le", "x2bgr10le"]]
    assert "gbrp" in groups[0] and "rgb24" in groups[0] and len(groups[0]) == 12 and len(groups[1]) == 6
    for names in groups:
        for pic, net in (((4, 12), None), ((5, 7), (8, 8))):
            H, W = pic
            r, g, b, fourth = _codes(R.FORMATS[names[0]].bits, H, W)
            y = torch.tensor(_values(*(net or pic))).to(DEV)
            first = None
            for name in names:
                x = rgb_to_input(torch.from_numpy(R.pack(r, g, b, name, fourth)).to(DEV), H, W, name, full_range=False, pad_to=net)
                codes = R.unpack(output_to_rgb(y, name, full_range=False, crop_to=pic if net else None).cpu().numpy(), H, W, name)[:3]
                first = first or (x, codes)
                assert arena.same_bits(x, first[0]), name
                assert all(np.array_equal(a, c) for a, c in zip(codes, first[1])), name


def test_alpha_filler_and_out():
    from bsvd_amd.frame_io import output_to_rgb, rgb_frame_bytes, rgb_to_input
    H, W = 4, 12
    y = torch.tensor(_values(H, W)).to(DEV)
    r, g, b, fourth = _codes(8, H, W)
    # alpha: the side plane out equals the codes in, alpha=None writes the maximum code, a wrong plane is refused
    x, alpha = rgb_to_input(torch.from_numpy(R.pack(r, g, b, "argb", fourth)).to(DEV), H, W, "argb", return_alpha=True)
    assert alpha.dtype == torch.uint8 and np.array_equal(alpha.cpu().numpy(), fourth)
    assert np.array_equal(R.unpack(output_to_rgb(y, "argb", alpha=alpha).cpu().numpy(), H, W, "argb")[3], fourth)
    assert set(R.unpack(output_to_rgb(y, "argb").cpu().numpy(), H, W, "argb")[3].ravel()) == {255}
    x16, a16 = rgb_to_input(torch.from_numpy(R.pack(*_codes(12, H, W)[:3], "gbrap12le", _codes(12, H, W)[3], junk="ones")).to(DEV), H, W,
                            "gbrap12le", return_alpha=True)
    assert a16.dtype == torch.uint16 and np.array_equal(a16.cpu().numpy().astype(np.int64), _codes(12, H, W)[3])
    with pytest.raises(ValueError, match="alpha"):
        output_to_rgb(y, "argb", alpha=a16)
    with pytest.raises(ValueError, match="alpha"):
        output_to_rgb(y, "argb", alpha=alpha[:, :2])
    # a filler reads as nothing and is written as all ones
    for junk in (np.zeros_like(fourth), fourth):
        assert arena.same_bits(rgb_to_input(torch.from_numpy(R.pack(r, g, b, "0bgr", junk)).to(DEV), H, W, "0bgr"), x)
    assert set(R.unpack(output_to_rgb(y, "0bgr").cpu().numpy(), H, W, "0bgr")[3].ravel()) == {255}
    # out=: the caller's padding survives; without out the padding of a pitched result is zero
    pitches, offsets, stride = _layouts(H, W, "gbrap")[1]
    out = torch.full((T, stride), 0xA5, dtype=torch.uint8, device=DEV)
    got = output_to_rgb(y, "gbrap", pitches=pitches, offsets=offsets, out=out, alpha=alpha)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), R.to_surface(y.cpu().numpy(), "gbrap", True, pitches, offsets, stride, alpha=fourth, fill=0xA5))
    fresh = output_to_rgb(y, "gbrap", pitches=pitches, offsets=offsets)
    assert fresh.shape == (T, rgb_frame_bytes(H, W, "gbrap", pitches, offsets))
    assert np.array_equal(fresh.cpu().numpy(), R.to_surface(y.cpu().numpy(), "gbrap", True, pitches, offsets, fill=0))


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import bsvd_amd
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32), 11)
    m = bsvd_amd.BSVD(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32, pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


def _frames(name, n, H, W, seed, dark_from=None):
    """natural arrays [n,H,W,4] of 8-bit pixels (as 257 x code at 16 bits: the same colours) with random alpha over the whole range;
    dark_from: the frames from that one on are a darker scene"""
    rs = np.random.RandomState(seed)
    px = rs.randint(0, 256, (n, H, W, 4))
    if dark_from is not None:
        px[dark_from:] //= 4
    if R.FORMATS[name].bits == 16:
        px[..., :3] *= 257
        px[..., 3] = rs.randint(0, 65536, (n, H, W))
    return px.astype(R.container(name))


def _direct(m, frames, name, pad, cuts=None):
    from bsvd_amd.frame_io import network_size, output_to_rgb, rgb_to_input
    n, H, W = frames.shape[:3]
    dev = torch.from_numpy(frames.view(np.uint8).reshape(n, -1)).to(DEV)
    x, alpha = rgb_to_input(dev, H, W, name, sigma=SIGMA, pad_to=network_size(H, W) if pad else None, return_alpha=True)
    y = m.clip_forward(x, **({} if cuts is None else dict(cuts=cuts)))
    return output_to_rgb(y, name, crop_to=(H, W) if pad else None, alpha=alpha).cpu().numpy().view(frames.dtype).reshape(frames.shape)


@pytest.mark.parametrize("name,size,pad", [("bgra", (16, 24), None), ("rgba64le", (16, 24), None), ("bgra", (5, 7), "reflect")])
def test_live_stream_carries_alpha_with_its_frame(model, name, size, pad):
    """frames byte-equal to rgb_to_input -> clip_forward -> output_to_rgb, the alpha of every returned frame its source frame's, through
    pipeline fill, steady state, a cut=True and flush()"""
    from bsvd_amd.pipeline import LiveStream
    live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt=name, pad=pad)
    n, cut = live.latency + live.depth + 3, 19                         # past one turn of the alpha ring
    frames = _frames(name, n, *size, seed=31)
    want = _direct(model, frames, name, pad, cuts=[cut])
    got = [r for r in (live.feed(fr, cut=(k == cut)) for k, fr in enumerate(frames)) if r is not None]
    assert len(got) == n - live.latency
    got += live.flush()
    assert len(got) == n and all(g.dtype == frames.dtype and g.shape == frames.shape[1:] for g in got)
    got = np.stack(got)
    assert np.array_equal(got[..., 3], frames[..., 3]), "alpha left its frame"
    assert np.array_equal(got, want)
    assert live._alpha.buf.shape[0] >= live.latency + live.depth


@pytest.mark.parametrize("name", ["bgra", "rgba64le"])
def test_clip_pipeline_carries_alpha(model, name):
    from bsvd_amd.pipeline import ClipPipeline
    for size, pad in (((16, 24), None), ((13, 22), "reflect")):
        clips = [_frames(name, 3 + (i % 2), *size, seed=21 + i) for i in range(3)]
        want = [_direct(model, c, name, pad) for c in clips]
        got = list(ClipPipeline(model, sigma=SIGMA, depth=2, pix_fmt=name, pad=pad).run(iter(clips)))
        assert len(got) == len(want)
        for g, w, c in zip(got, want, clips):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) and np.array_equal(g[..., 3], c[..., 3])


@pytest.mark.parametrize("name", ["bgra", "rgba64le"])
def test_auto_sigma_and_auto_cuts_see_the_rgb24_pixels(model, name):
    """sigma='auto' and cuts='auto' read the converted tensor: the same pixels as rgb24 give the same estimates, scores and frames"""
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    H, W = 16, 24
    frames = _frames(name, 20, H, W, seed=51, dark_from=9)            # a scene change for the detector
    order = R.FORMATS[name].order
    rgb24 = np.ascontiguousarray(np.stack([frames[..., order.index(c)] for c in "rgb"], axis=-1) // (257 if R.FORMATS[name].bits == 16 else 1)).astype(np.uint8)
    seen = []
    for pix_fmt, fed in ((name, frames), ("rgb24", rgb24)):
        live = LiveStream(model, sigma="auto", cuts="auto", depth=2, pix_fmt=pix_fmt)
        outs, trace = [], []
        for fr in fed:
            r = live.feed(fr)
            trace.append((live.last_sigma, live.last_cut_score, live.last_cut))
            if r is not None:
                outs.append(r)
        outs += live.flush()
        seen.append((np.stack(outs), trace))
    (a, ta), (b, tb) = seen
    assert ta == tb
    top = 65535 if R.FORMATS[name].bits == 16 else 255
    back = np.stack([a[..., order.index(c)] for c in "rgb"], axis=-1)
    if top == 255:
        assert np.array_equal(back, b)
    else:       # the same values v at 16 bits: |rint(65535 v) / 257 - 255 v| <= 0.5 / 257 (+ fp32 rounding of the product) and |255 v - rint(255 v)| <= 0.5
        assert np.abs(back / 257.0 - b).max() <= 0.5 + 1.0 / 257
    assert np.array_equal(a[..., order.index("a")], frames[..., order.index("a")])
    pa, pb = (ClipPipeline(model, sigma="auto", cuts="auto", pix_fmt=p) for p in (name, "rgb24"))
    ra, rb = pa.submit(frames[:12]).finish(), pb.submit(rgb24[:12]).finish()
    assert pa.last_cuts == pb.last_cuts
    assert np.array_equal(ra[..., order.index("a")], frames[:12][..., order.index("a")])
    if top == 255:
        assert np.array_equal(np.stack([ra[..., order.index(c)] for c in "rgb"], axis=-1), rb)
