"""The output finish on the device (bsvd_amd/csrc/frame_finish.hip: bsvd_blend_planar; the `_d` encoders of frame_yuv.hip / frame_rgb.hip;
frame_io.blend_output / output_to_*(dither=) and the pipelines' strength / dither) against the numpy model tests/finish_model.py.

Pictures are 3 frames of 10 x 22, 12 x 18 and 16 x 32 inside tensors of 16 x 24 and 16 x 32: rows that end in part items of two columns, a
crop both ways, more than one item row.  Surfaces run tight and pitched with gaps, inside allocations prefilled with 0xA5 and 0x5A: the same
bytes from both prefills mean every sample was written, and every other byte keeps its prefill.  The fp32 tensors live between NaN guards
(tests/arena.py), their pad rows and columns hold NaN.  RGB is compared byte for byte (the model is the device's arithmetic); YUV code for
code except at near-ties of the float64 model, where a step of 1 is accepted -- the rule of the YUV encoders' own tests."""
import ctypes

import numpy as np
import pytest
import torch

import arena
import finish_model as F
import rgb_surface_model as R
import yuv_model as M
import yuv_surface_model as S
import test_gpu_rgb as TR
import test_gpu_yuv_formats as TY
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = F.T
GUARD = 64
SIGMA = TR.SIGMA
RGB_NAMES = TR.NAMES                         # every name of rgb_surface_model.FORMATS: all nine encoder instantiations
YUV_NAMES = TY.NAMES                         # the ten surfaces of bsvd_planar_to_yuv; nv12 / p010 go through bsvd_planar_to_yuv420
MODES = [("ordered", F.ORDERED), ("random", F.RANDOM)]


def _lib():
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    return _lib, require_hip()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tensor(net, pic):
    """the shared values with NaN in the pad rows and columns, in an arena between NaN guards -> (host array, arena)"""
    (H, W), (Hp, Wp) = pic, net
    y = F.values(Hp, Wp).copy()
    y[:, :, H:, :] = np.nan
    y[:, :, :, W:] = np.nan
    return y, arena.reserve(y.shape, 0, fill=0xFF, device=DEV).write(torch.from_numpy(y))


def _alloc(T_, stride, fill):
    big = torch.full((GUARD + T_ * stride + GUARD,), fill, dtype=torch.uint8, device=DEV)
    return big, big.data_ptr() + GUARD


def _dither(mode, frame0=F.FRAME0):
    _l, _ = _lib()
    return _l.BsvdDither(mode=mode, seed=F.SEED, frame0=frame0)


def _framed(buf, fill):
    return np.concatenate([np.full(GUARD, fill, np.uint8), buf.reshape(-1), np.full(GUARD, fill, np.uint8)])


# ---- the blend -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", [(16, 32), (16, 24)])
@pytest.mark.parametrize("off", [0, 1], ids=["float4", "scalar"])
def test_blend_is_the_model_bit_for_bit(net, off):
    """strengths (1,1), (0,0), (0.5,0.5), (0.3,0.9), (1,0); x frames 4 planes apart with NaN in the fourth, y frames 3 planes and 8 floats
    apart; aligned (the float4 path) and one float off (the scalar path); nothing outside y's elements is written, x stays as it was"""
    _l, lib = _lib()
    Hp, Wp = net
    rs = np.random.RandomState(Hp + Wp)
    y0 = rs.uniform(-0.2, 1.2, (T, 3, Hp, Wp)).astype(np.float32)
    x0 = rs.uniform(-0.2, 1.2, (T, 3, Hp, Wp)).astype(np.float32)
    w = F.LUMA_W["bt601"]
    cw = (ctypes.c_float * 3)(*w)
    for s_l, s_c in ((1.0, 1.0), (0.0, 0.0), (0.5, 0.5), (0.3, 0.9), (1.0, 0.0)):
        ya = arena.reserve((T, 3, Hp, Wp), 8, fill=0xFF, device=DEV)
        xa = arena.reserve((T, 4, Hp, Wp), 0, fill=0xFF, device=DEV)
        if off:
            ya = arena.Arena(ya.size, ya.stride, ya.offset + 1, ya.buf.numel() // 4, 0xFF, DEV)
            xa = arena.Arena(xa.size, xa.stride, xa.offset + 1, xa.buf.numel() // 4, 0xFF, DEV)
        ya.write(torch.from_numpy(y0))
        xa.view()[:, :3].copy_(torch.from_numpy(x0).to(DEV))                 # the noise-map plane stays NaN: never read
        assert (ya.ptr % 16 == 0) == (off == 0)
        x_before = xa.buf.clone()
        _l.check(lib.bsvd_blend_planar(ya.ptr, ya.frame_stride, xa.ptr, xa.frame_stride, T, Hp, Wp, s_l, s_c, cw, None), "bsvd_blend_planar")
        torch.cuda.synchronize()
        got = ya.logical().cpu().numpy()
        want = F.blend(y0, x0, s_l, s_c, w)
        assert ya.slack_intact(), ya.slack_damage()
        assert torch.equal(xa.buf, x_before)
        assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want)), (s_l, s_c, int((_bits(got) != _bits(want)).sum()))
        if (s_l, s_c) == (1.0, 1.0):
            assert np.array_equal(_bits(got), _bits(y0))
        if (s_l, s_c) == (0.0, 0.0):
            assert np.array_equal(_bits(got), _bits(x0))


def test_blend_output_checks_and_blends_in_place():
    from bsvd_amd.frame_io import blend_output
    y = torch.rand((2, 3, 8, 12), device=DEV)
    x = torch.rand((2, 4, 8, 12), device=DEV)
    y0 = y.clone()
    assert blend_output(y, x, 1.0).data_ptr() == y.data_ptr() and torch.equal(y, y0)
    want = F.blend(y0.cpu().numpy(), x.cpu().numpy(), 0.25, 0.75, F.LUMA_W["bt2020"])
    assert np.array_equal(_bits(blend_output(y, x, (0.25, 0.75), matrix="bt2020").cpu().numpy()), _bits(want))
    assert torch.equal(blend_output(y, x, 0.0), x[:, :3])
    for bad in (dict(strength=1.5), dict(strength=(0.5, -1)), dict(strength=0.5, matrix="bt470")):
        with pytest.raises(ValueError):
            blend_output(y, x, **bad)
    with pytest.raises(ValueError, match="blend_output"):
        blend_output(y, x[:, :, :4], 0.5)


# ---- the RGB encoder -------------------------------------------------------------------------------------------------------------------------
def _encode_rgb(src, net, pic, name, full_range, layout, dither, frames=T, alpha=None, first=0):
    """bsvd_planar_to_rgb (dither None) or bsvd_planar_to_rgb_d into 0xA5- and 0x5A-prefilled allocations -> the two allocations whole"""
    _l, lib = _lib()
    (H, W), (Hp, Wp) = pic, net
    stride = layout[2] or R.frame_bytes(H, W, name)
    s = TR._surface(name, full_range, *layout)
    out = []
    for fill in (0xA5, 0x5A):
        big, ptr = _alloc(frames, stride, fill)
        sp = src.ptr + first * 3 * Hp * Wp * 4
        ap = None if alpha is None else alpha.data_ptr()
        if dither is None:
            _l.check(lib.bsvd_planar_to_rgb(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(s), ap, None), "bsvd_planar_to_rgb")
        else:
            _l.check(lib.bsvd_planar_to_rgb_d(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(s), ap, ctypes.byref(dither), None), "bsvd_planar_to_rgb_d")
        torch.cuda.synchronize()
        out.append(big.cpu().numpy())
    return out


@pytest.mark.parametrize("name", RGB_NAMES)
def test_rgb_dither_is_the_model_byte_for_byte_and_none_is_the_plain_encoder(name):
    """every instantiation, both ranges (limited: both legal ends are met), tight and pitched; alpha codes pass untouched; frame0 = 5"""
    for pic, net in F.PICTURES:
        H, W = pic
        y, src = _tensor(net, pic)
        alpha = dev_alpha = None
        if R.has_alpha(name):
            alpha = np.random.RandomState(H + W).randint(0, 1 << 16, (T, H, W)).astype(R.container(name))
            dev_alpha = torch.from_numpy(alpha.view(np.uint8).reshape(T, H, -1).copy()).to(DEV)
        for full_range in (True, False):
            for layout in TR._layouts(H, W, name):
                plain = _encode_rgb(src, net, pic, name, full_range, layout, None, alpha=dev_alpha)
                none = _encode_rgb(src, net, pic, name, full_range, layout, _dither(F.NONE), alpha=dev_alpha)
                assert all(np.array_equal(a, b) for a, b in zip(plain, none)), (pic, full_range, layout)
                for mode_name, mode in MODES:
                    got = _encode_rgb(src, net, pic, name, full_range, layout, _dither(mode), alpha=dev_alpha)
                    for big, fill in zip(got, (0xA5, 0x5A)):
                        want = F.rgb_to_surface(y, name, full_range, *layout, crop_to=pic, alpha=alpha, fill=fill, mode=mode_name, seed=F.SEED,
                                                frame0=F.FRAME0)
                        assert np.array_equal(big, _framed(want, fill)), (pic, full_range, layout, mode_name, fill)
                    assert not np.array_equal(got[0], plain[0])
                    if not full_range:
                        r, g, b, _, _ = R.unpack(got[0][GUARD:-GUARD].reshape(T, -1), H, W, name, layout[0], layout[1])
                        s = 1 << (R.FORMATS[name].bits - 8)
                        assert min(r.min(), g.min(), b.min()) == 16 * s and max(r.max(), g.max(), b.max()) == 235 * s
        assert src.slack_intact()


# ---- the YUV encoders ------------------------------------------------------------------------------------------------------------------------
def _yuv_surface_struct(pix_fmt, matrix, full_range, chroma, pitches, offsets, stride):
    _l, _ = _lib()
    sub, layout, bits, high = _l.YUV_FORMATS[pix_fmt]
    s = _l.BsvdYuvSurface(subsampling=sub, layout=layout, bits=bits, high_bits=high, matrix=_l.MATRIX[matrix], full_range=int(full_range),
                          chroma=_l.CHROMA[chroma])
    s.pitch[:] = tuple(pitches or ()) + (0,) * (3 - len(pitches or ()))
    s.offset[:] = tuple(offsets or ()) + (0,) * (3 - len(offsets or ()))
    s.frame_stride = stride or 0
    return s


def _encode_yuv(src, net, pic, pix_fmt, kw, layout, dither, frames=T, first=0):
    """bsvd_planar_to_yuv_crop(_d) / bsvd_planar_to_yuv420_crop(_d) -> the two allocations whole (layout: (pitches, offsets, stride); nv12 /
    p010: ((row_pitch,), None, stride))"""
    _l, lib = _lib()
    (H, W), (Hp, Wp) = pic, net
    sp = src.ptr + first * 3 * Hp * Wp * 4
    out = []
    for fill in (0xA5, 0x5A):
        if pix_fmt in M.BITS:
            pitch = layout[0][0] if layout[0] else 0
            stride = layout[2] or M.frame_bytes(H, W, pix_fmt, pitch or None)
            d = _l.BsvdYuvDesc(pix_fmt=_l.PIX_FMT[pix_fmt], matrix=_l.MATRIX[kw["matrix"]], full_range=int(kw["full_range"]),
                               chroma=_l.CHROMA[kw["chroma"]], row_pitch=pitch, frame_stride=layout[2] or 0)
            big, ptr = _alloc(frames, stride, fill)
            if dither is None:
                _l.check(lib.bsvd_planar_to_yuv420_crop(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(d), None), "bsvd_planar_to_yuv420_crop")
            else:
                _l.check(lib.bsvd_planar_to_yuv420_crop_d(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(d), ctypes.byref(dither), None),
                         "bsvd_planar_to_yuv420_crop_d")
        else:
            stride = layout[2] or S.frame_bytes(H, W, pix_fmt)
            s = _yuv_surface_struct(pix_fmt, kw["matrix"], kw["full_range"], kw["chroma"], *layout)
            big, ptr = _alloc(frames, stride, fill)
            if dither is None:
                _l.check(lib.bsvd_planar_to_yuv_crop(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(s), None), "bsvd_planar_to_yuv_crop")
            else:
                _l.check(lib.bsvd_planar_to_yuv_crop_d(sp, ptr, frames, Hp, Wp, H, W, ctypes.byref(s), ctypes.byref(dither), None),
                         "bsvd_planar_to_yuv_crop_d")
        torch.cuda.synchronize()
        out.append(big.cpu().numpy())
    return out


def _yuv_layouts(H, W, pix_fmt):
    if pix_fmt in M.BITS:
        sb = 2 if pix_fmt == "p010" else 1
        pitch = (W * sb + 63) // 64 * 64 + 64
        return [(None, None, None), ((pitch,), None, M.frame_bytes(H, W, pix_fmt, pitch) + 128)]
    return TY._layouts(H, W, pix_fmt)


def _yuv_unpack(big, frames, H, W, pix_fmt, layout, fill):
    """-> ([Y, Cb, Cr] codes, ok: every byte that is no sample keeps the prefill and no ignored bit is set)"""
    surf = big[GUARD:-GUARD].reshape(frames, -1)
    guards = (big[:GUARD] == fill).all() and (big[-GUARD:] == fill).all()
    if pix_fmt in M.BITS:
        pitch = layout[0][0] if layout[0] else None
        Y, Cb, Cr = M.unpack(surf, H, W, pix_fmt, pitch)[:3]
        mask = M.sample_mask(frames, H, W, pix_fmt, pitch, surf.shape[1])
        return [Y, Cb, Cr], bool(guards and (surf[~mask] == fill).all())
    Y, Cb, Cr, ignored = S.unpack(surf, H, W, pix_fmt, layout[0], layout[1])
    mask = S.sample_mask(frames, H, W, pix_fmt, layout[0], layout[1], surf.shape[1])
    return [Y, Cb, Cr], bool(guards and ignored == 0 and (surf[~mask] == fill).all())


@pytest.mark.parametrize("pix_fmt", YUV_NAMES + ["nv12", "p010"])
def test_yuv_dither_is_the_model_and_none_is_the_plain_encoder(pix_fmt):
    """every format (4:2:0, 4:2:2 planar / semi-planar / packed, 4:4:4; 8 and 10 bit), limited range with both legal ends met and full range,
    both chroma filters, tight and pitched, frame0 = 5.  Subsampled chroma is dithered on the chroma grid: the luma-grid mutant of
    tests/test_finish_cpu.py fails these inputs."""
    codes = F.yuv420_codes if pix_fmt in M.BITS else F.yuv_codes
    bits = M.BITS[pix_fmt] if pix_fmt in M.BITS else S.FORMATS[pix_fmt].bits
    ends = [set(), set()]                                   # the extreme luma and chroma codes met at limited range, over the pictures
    for pic, net in F.PICTURES:
        H, W = pic
        y, src = _tensor(net, pic)
        for kw in (dict(matrix="bt709", full_range=False, chroma="linear"), dict(matrix="bt601", full_range=True, chroma="nearest")):
            for layout in _yuv_layouts(H, W, pix_fmt):
                plain = _encode_yuv(src, net, pic, pix_fmt, kw, layout, None)
                none = _encode_yuv(src, net, pic, pix_fmt, kw, layout, _dither(F.NONE))
                assert all(np.array_equal(a, b) for a, b in zip(plain, none)), (pic, kw, layout)
                for mode_name, mode in MODES:
                    want, ties = codes(y[..., :H, :W], pix_fmt, mode=mode_name, seed=F.SEED, frame0=F.FRAME0, **kw)
                    assert sum(int(t.sum()) for t in ties) <= 0.01 * sum(t.size for t in ties)
                    got = _encode_yuv(src, net, pic, pix_fmt, kw, layout, _dither(mode))
                    planes = []
                    for big, fill in zip(got, (0xA5, 0x5A)):
                        p, ok = _yuv_unpack(big, T, H, W, pix_fmt, layout, fill)
                        assert ok, (pic, kw, layout, mode_name, fill)
                        assert F.mismatches(p, want, ties) == 0, (pic, kw, layout, mode_name, F.mismatches(p, want, ties))
                        planes.append(p)
                    assert all(np.array_equal(a, b) for a, b in zip(*planes)), "a sample was not written"
                    if not kw["full_range"]:
                        ends[0] |= {int(planes[0][0].min()), int(planes[0][0].max())}
                        ends[1] |= {int(v) for c in planes[0][1:] for v in (c.min(), c.max())}
        assert src.slack_intact()
    s = 1 << (bits - 8)
    assert {16 * s, 235 * s} <= ends[0] and {16 * s, 240 * s} <= ends[1] and min(ends[0] | ends[1]) == 16 * s and max(ends[1]) == 240 * s


@pytest.mark.parametrize("name", ["nv12", "yuv422p10le", "uyvy422", "yuv444p", "bgra", "x2rgb10le", "gbrp16le"])
def test_one_call_of_three_frames_is_three_calls_with_the_stream_index(name):
    """random dither hashes frame0 + f: T = 3 at frame0 = 5 gives the bytes of three calls at frame0 = 5, 6, 7, and not those of three calls
    at frame0 = 5"""
    pic, net = F.PICTURES[0]
    H, W = pic
    y, src = _tensor(net, pic)
    kw = dict(matrix="bt709", full_range=False, chroma="linear")
    rgb = name in R.FORMATS

    def run(frames, first, frame0):
        d = _dither(F.RANDOM, frame0)
        big = (_encode_rgb(src, net, pic, name, True, (None, None, None), d, frames, first=first) if rgb
               else _encode_yuv(src, net, pic, name, kw, (None, None, None), d, frames, first=first))[0]
        return big[GUARD:-GUARD].reshape(frames, -1)

    whole = run(T, 0, F.FRAME0)
    singles = np.concatenate([run(1, t, F.FRAME0 + t) for t in range(T)])
    assert np.array_equal(whole, singles)
    local = np.concatenate([run(1, t, F.FRAME0) for t in range(T)])
    assert np.array_equal(whole[0], local[0]) and not np.array_equal(whole[1:], local[1:])


def test_frame_io_passes_dither_through_and_defaults_are_the_plain_calls():
    from bsvd_amd.frame_io import output_to_rgb, output_to_yuv, output_to_yuv420
    pic, net = F.PICTURES[0]
    y = torch.from_numpy(F.values(*net)).to(DEV)
    kw = dict(dither="random", dither_seed=F.SEED, frame0=F.FRAME0)
    got = output_to_rgb(y, "bgra", crop_to=pic, **kw).cpu().numpy()
    assert np.array_equal(got, F.rgb_to_surface(F.values(*net), "bgra", crop_to=pic, mode="random", seed=F.SEED, frame0=F.FRAME0))
    for fn, fmt, codes, unpack in ((output_to_yuv, "yuv420p", F.yuv_codes, lambda b: S.unpack(b, *pic, "yuv420p")[:3]),
                                   (output_to_yuv420, "nv12", F.yuv420_codes, lambda b: M.unpack(b, *pic, "nv12")[:3])):
        want, ties = codes(F.values(*net)[..., :pic[0], :pic[1]], fmt, mode="random", seed=F.SEED, frame0=F.FRAME0)
        assert F.mismatches(unpack(fn(y, pix_fmt=fmt, crop_to=pic, **kw).cpu().numpy()), want, ties) == 0
        assert torch.equal(fn(y, pix_fmt=fmt, crop_to=pic), fn(y, pix_fmt=fmt, crop_to=pic, dither=None, dither_seed=3, frame0=9))
        full = y[..., :16, :24].contiguous()                                  # without crop_to: the `_d` entry point at Hp == H, Wp == W
        assert not torch.equal(fn(full, pix_fmt=fmt), fn(full, pix_fmt=fmt, dither="ordered"))
    with pytest.raises(ValueError, match="dither"):
        output_to_rgb(y, "bgra", dither="floyd")


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------------------
def _frames(name, n, H, W, seed):
    """natural arrays of full-range codes over the whole code range: [n,H,W,4] for bgra (alpha included), [n,H,W,3] uint16 for rgb48le"""
    rs = np.random.RandomState(seed)
    if name == "bgra":
        return rs.randint(0, 256, (n, H, W, 4)).astype(np.uint8)
    return rs.randint(0, 65536, (n, H, W, 3)).astype(np.uint16)


def _by_hand(m, frames, name, cuts, strength, dither, frame0=0, sigma=SIGMA, size=None, pad=None, seed=F.SEED, info=None):
    """*_to_input -> clip_forward -> blend_output -> output_to_*, with the stream's frame indices, on the default stream and synchronised.
    ``name``: an RGB surface (frames: natural arrays [n,H,W,c]), 'rgb24', or a surface of bsvd_yuv_to_planar with the colour defaults
    (frames: [n, samples] with ``size`` = (H, W)).  ``pad``: 'reflect'.  ``cuts``: the scene starts, or 'auto': frame_io.scene_cuts on
    the converted tensor.  ``sigma``: a number or 'auto'.  ``info`` (a dict): gets 'cuts' (the starts used) and 'sigma' (estimate_sigma
    per frame, as floats)."""
    from bsvd_amd.frame_io import (blend_output, estimate_sigma, frames_to_input, network_size, output_to_frames, output_to_rgb, output_to_yuv,
                                   rgb_to_input, scene_cuts, yuv_to_input)
    n = frames.shape[0]
    H, W = frames.shape[1:3] if size is None else size
    pad_to, crop_to = (network_size(H, W), (H, W)) if pad else (None, None)
    dev = torch.from_numpy(frames.view(np.uint8).reshape(n, -1)).to(DEV)
    alpha = None
    if name in YUV_NAMES:
        x = yuv_to_input(dev, H, W, name, sigma=sigma, pad_to=pad_to)
    elif name == "rgb24":
        x = frames_to_input(dev.view(n, H, W, 3), sigma, pad_to=pad_to)
    elif R.has_alpha(name):
        x, alpha = rgb_to_input(dev, H, W, name, sigma=sigma, pad_to=pad_to, return_alpha=True)
    else:
        x = rgb_to_input(dev, H, W, name, sigma=sigma, pad_to=pad_to)
    if isinstance(cuts, str):
        cuts = scene_cuts(x, picture=(H, W))
    if info is not None:
        info["cuts"] = list(cuts or [])
        info["sigma"] = [float(v) for v in estimate_sigma(x, picture=(H, W)).cpu()]
    y = m.clip_forward(x, **({} if not cuts else dict(cuts=cuts))).float().contiguous()
    if strength is not None:
        blend_output(y, x, strength)
    if name in YUV_NAMES:
        out = output_to_yuv(y, name, crop_to=crop_to, dither=dither, dither_seed=seed, frame0=frame0)
    elif name == "rgb24" and dither is None:
        out = output_to_frames(y, crop_to=crop_to)
    else:
        out = output_to_rgb(y, name, crop_to=crop_to, alpha=alpha, dither=dither, dither_seed=seed, frame0=frame0)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(frames.dtype).reshape(frames.shape)


def _stream(live, frames, cut=None):
    got = [r for r in (live.feed(fr, cut=(k == cut)) for k, fr in enumerate(frames)) if r is not None]
    return np.stack(got + live.flush())


@pytest.mark.parametrize("name", ["bgra", "rgb48le"])
def test_strength_zero_returns_the_source_bytes(model, name):     # noqa: F811
    """strength = 0: every frame comes back as it went in, alpha included, through pipeline fill, a cut=True, a flush() and a second stream
    on the same object, with ordered dither on as well -- the blend's exact end, the round trip of every full-range code, and the
    whole-code property of the dither, end to end"""
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    H, W = 16, 24
    for dither in (None, "ordered"):
        live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt=name, strength=0.0, dither=dither, dither_seed=F.SEED)
        n = live.latency + live.depth + 3                                     # past one turn of the source ring
        frames = _frames(name, n, H, W, seed=41)
        assert np.array_equal(_stream(live, frames, cut=19), frames)
        assert live._source.buf.shape == (live.latency + live.depth, 1, 3, H, W)
        again = _frames(name, 5, H, W, seed=42)                               # after the flush: the ring starts over
        assert np.array_equal(_stream(live, again), again)
        clips = [_frames(name, 3 + (i % 2), H, W, seed=43 + i) for i in range(3)]
        got = list(ClipPipeline(model, sigma=SIGMA, depth=2, pix_fmt=name, strength=0.0, dither=dither).run(iter(clips)))
        assert all(np.array_equal(g, c) for g, c in zip(got, clips))


@pytest.mark.parametrize("name,depth,overlap", [("bgra", 2, None), ("rgb48le", 1, False)])
def test_strength_and_random_dither_equal_the_steps_by_hand(model, name, depth, overlap):     # noqa: F811
    """strength = (0.4, 1.0), dither = 'random': LiveStream (feed_overlapped and feedin_one_element) and ClipPipeline give the bytes of
    blend_output + output_to_rgb applied to clip_forward's result with the stream's frame indices; the index restarts at flush()"""
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    H, W = 16, 24
    kw = dict(strength=(0.4, 1.0), dither="random", dither_seed=F.SEED)
    live = LiveStream(model, sigma=SIGMA, depth=depth, overlap_blocks=overlap, pix_fmt=name, **kw)
    frames = _frames(name, live.latency + live.depth + 3, H, W, seed=51)
    want = _by_hand(model, frames, name, [19], (0.4, 1.0), "random")
    assert np.array_equal(_stream(live, frames, cut=19), want)
    assert not np.array_equal(want, _by_hand(model, frames, name, [19], None, None))
    short = frames[:6]
    assert np.array_equal(_stream(live, short), _by_hand(model, short, name, None, (0.4, 1.0), "random"))          # frame0 is 0 again
    clips = [_frames(name, 3 + (i % 2), H, W, seed=61 + i) for i in range(3)]
    starts = np.cumsum([0] + [len(c) for c in clips])
    got = list(ClipPipeline(model, sigma=SIGMA, depth=2, pix_fmt=name, **kw).run(iter(clips)))
    for g, c, f0 in zip(got, clips, starts):
        assert np.array_equal(g, _by_hand(model, c, name, None, (0.4, 1.0), "random", frame0=int(f0)))


def test_yuv_stream_blends_with_its_matrix_and_dithers(model):     # noqa: F811
    """a YUV stream: the blend's luma weights are the stream's matrix, the chroma planes are dithered on their own grid"""
    from bsvd_amd.frame_io import blend_output, output_to_yuv, yuv_to_input
    from bsvd_amd.pipeline import LiveStream
    H, W = 16, 24
    colour = dict(matrix="bt601", full_range=False, chroma="linear")
    live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt="yuv420p", frame_shape=(H, W), colour=colour, strength=(0.2, 0.8), dither="random",
                      dither_seed=F.SEED)
    n = live.latency + 4
    rs = np.random.RandomState(71)
    frames = rs.randint(16, 236, (n, H * W * 3 // 2)).astype(np.uint8)
    got = _stream(live, frames)
    x = yuv_to_input(torch.from_numpy(frames).to(DEV), H, W, "yuv420p", sigma=SIGMA, **colour)
    y = model.clip_forward(x).float().contiguous()
    blend_output(y, x, (0.2, 0.8), matrix="bt601")
    want = output_to_yuv(y, "yuv420p", dither="random", dither_seed=F.SEED, frame0=0, **colour).cpu().numpy()
    assert np.array_equal(got, want)


def test_steady_state_allocates_nothing_and_defaults_are_untouched(model):     # noqa: F811
    from bsvd_amd.pipeline import LiveStream
    H, W = 16, 24
    frames = TR._frames("bgra", 24, H, W, seed=81)
    plain = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt="bgra")
    new = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt="bgra", strength=1.0, dither=None, dither_seed=0)
    want = _stream(plain, frames)
    assert np.array_equal(_stream(new, frames), want) and np.array_equal(want, TR._direct(model, frames, "bgra", None))
    assert new._source is None and not new.finish.blends and new.finish.dither_kw(1) == {}
    live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt="bgra", strength=(0.5, 0.9), dither="ordered")
    period = live.latency + live.depth
    for k in range(period + 2):                                                   # the first ring period, graphs captured
        live.feed(frames[k % len(frames)])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    seen = set()
    for k in range(40):
        assert live.feed(frames[k % len(frames)]) is not None
        seen.add(torch.cuda.memory_allocated())
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and len(seen) <= 2, (before, sorted(seen))
    live.flush()
