"""The output finish without a device: the properties of the blend and of both dithers on the numpy model (tests/finish_model.py, written
from include/bsvd_hip.h), the mutants the device comparison of tests/test_gpu_finish.py must catch, the bookkeeping of LiveStream's source
ring, and the refusals of the new entry points (no kernel is launched)."""
import ctypes

import numpy as np
import pytest

import finish_model as F
import yuv_surface_model as S

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- the blend -------------------------------------------------------------------------------------------------------------------------------
def _random_fp32(shape, seed):
    """finite fp32 over many binades, both signs, most of it far outside [0,1]"""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(shape) * np.exp2(rs.randint(-20, 21, shape))).astype(f32)


def test_blend_ends_are_exact():
    y, x = _random_fp32((2, 3, 8, 12), 1), _random_fp32((2, 4, 8, 12), 2)
    for w in F.LUMA_W.values():
        assert np.array_equal(_bits(F.blend(y, x, 1.0, 1.0, w)), _bits(y))
        assert np.array_equal(_bits(F.blend(y, x, 0.0, 0.0, w)), _bits(x[:, :3]))
        for s in (0.5, 0.3, 0.7, 0.999, 2.0 ** -20):
            assert np.array_equal(_bits(F.blend(y, x, s, s, w)), _bits(F.lerp(y, x, s))), s
    # ... which y + (1 - s)(x - y) has not: at s = 0 it misses x for most values
    naive = (y + f32(1) * (x[:, :3] - y)).astype(f32)
    assert (_bits(naive) != _bits(x[:, :3])).mean() > 0.05
    # luma and chroma strengths do different things: (1, 0) keeps the network's luma of the difference, (0, 1) its chroma
    a, b = F.blend(y, x, 1.0, 0.0), F.blend(y, x, 0.0, 1.0)
    assert not np.array_equal(a, b)


def test_blend_luma_strength_moves_luma_only():
    """on values in [0,1]: with s_chroma = 1 the result differs from y by the same amount in R, G and B (a pure luma step)"""
    rs = np.random.RandomState(3)
    y, x = rs.uniform(0, 1, (1, 3, 4, 8)).astype(f32), rs.uniform(0, 1, (1, 3, 4, 8)).astype(f32)
    out = F.blend(y, x, 0.25, 1.0).astype(np.float64)
    step = out - y
    assert np.abs(step - step[:, :1]).max() < 1e-6 and np.abs(step).max() > 1e-2
    w = np.array(F.LUMA_W["bt709"])[None, :, None, None]
    want = 0.75 * ((x.astype(np.float64) - y) * w).sum(axis=1)
    assert np.abs(step[:, 0] - want).max() < 1e-6


# ---- d ---------------------------------------------------------------------------------------------------------------------------------------
def test_bayer_matrix_and_shifts():
    assert sorted(F.BAYER8.ravel()) == list(range(64))
    assert list(F.BAYER8[0]) == [0, 32, 8, 40, 2, 34, 10, 42]               # the row the header quotes
    # the closed form of frame_finish_items.h (bayer8): the bits of x ^ y and y interleaved
    for yy in range(8):
        for xx in range(8):
            c = xx ^ yy
            v = ((c & 1) << 5) | ((yy & 1) << 4) | ((c & 2) << 2) | ((yy & 2) << 1) | ((c & 4) >> 1) | ((yy & 4) >> 2)
            assert v == F.BAYER8[yy, xx], (yy, xx)
    assert len(set(F.SHIFTS)) == 3
    planes = [F.d_plane("ordered", c, 8, 8) for c in range(3)]
    for i in range(3):
        for j in range(i):
            assert (planes[i] != planes[j]).mean() > 0.4


def test_d_lies_in_the_open_interval():
    d = F.d_ordered_entry(np.arange(64))
    assert d.dtype == f32 and d.min() == f32(-0.5 + 1 / 128) and d.max() == f32(0.5 - 1 / 128) and np.all(np.abs(d) < 0.5)
    assert np.array_equal(d.astype(np.float64), (np.arange(64) + 0.5) / 64 - 0.5)                # every step exact
    h = np.array([0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 255, 256], np.uint64)
    d = F.d_of_hash(h)
    assert d.dtype == f32 and np.all(np.abs(d) < 0.5) and d[0] == -F.RANDOM_MAX and d[1] == F.RANDOM_MAX
    # before the limit, d is the header's ((h >> 8) + 0.5) 2^-24 - 0.5 exactly
    hh = np.random.RandomState(0).randint(0, 2 ** 32, 4096).astype(np.uint64)
    exact = ((hh >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 - 0.5
    assert np.array_equal(F.d_of_hash(hh).astype(np.float64), np.clip(exact, -float(F.RANDOM_MAX), float(F.RANDOM_MAX)))
    # the literal fp32 form reaches the closed end: why the header rearranges it
    top = f32(2 ** 24 - 1) + f32(0.5)
    assert top * f32(2.0 ** -24) - f32(0.5) == f32(0.5)


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_whole_codes_are_never_moved(bits):
    """every whole code, both modes, both rounding orders, the extreme hash values included: t + d is one fp32 addition, and the limit of the
    random d is what keeps its ROUNDED sum off the tie at the high codes"""
    codes = np.arange(1 << bits)
    t = codes.astype(f32)[:, None]
    ds = [F.d_ordered_entry(np.arange(64)), F.d_of_hash(np.array([0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1], np.uint64)),
          F.d_plane("random", 1, 8, 32, seed=F.SEED, frame=F.FRAME0).ravel()]
    for d in ds:
        for rgb_order in (False, True):
            got = F.quantise(t, d[None, :], 0, (1 << bits) - 1, rgb_order)
            assert np.array_equal(got, np.broadcast_to(codes[:, None], got.shape)), (bits, rgb_order)
    # ... and a code that went through the decode (code / top) and the encoder's scale, which can leave t one fp32 spacing off the code
    top = f32((1 << bits) - 1)
    t = ((codes.astype(f32) / top) * top)[:, None]
    for d in ds[:2]:
        got = F.quantise(t, d[None, :], 0, (1 << bits) - 1, True)
        assert np.array_equal(got, np.broadcast_to(codes[:, None], got.shape)), bits
    if bits == 16:      # without the limit the property fails at 16 bits: d = 0.5 - 2^-25 added to an odd code above 2^15 rounds to the tie
        raw = (f32(2 ** 23 - 1) + f32(0.5)) * f32(2.0 ** -24)
        assert np.rint(f32(32769) + raw) == 32770


def test_ordered_dither_debands_and_plain_rounding_does_not():
    """an aligned 8 x 8 tile of a constant t: the mean of the codes is within 1/64 code of t (64 equally spaced thresholds: 1/128 worst case,
    the rest margin for ties), for 257 values of t across two codes, for every component's shift; round-to-nearest misses by up to 0.5"""
    ts = (f32(100) + np.arange(257, dtype=f32) / f32(128))
    worst_plain = 0.0
    for comp in range(3):
        d = F.d_plane("ordered", comp, 8, 8)
        for t in ts:
            tile = np.full((8, 8), t, f32)
            mean = F.quantise(tile, d, 0, 255).mean()
            assert abs(mean - float(t)) <= 1 / 64, (comp, float(t), mean)
            worst_plain = max(worst_plain, abs(F.quantise(tile, np.zeros((8, 8), f32), 0, 255).mean() - float(t)))
    assert worst_plain >= 0.49


def test_random_dither_is_unbiased_for_the_seed_used():
    """64 x 64 constant field, the seed of the device tests: mean within 0.04 code of t (5 sigma of 0.5 / sqrt(4096))"""
    for comp in range(3):
        d = F.d_plane("random", comp, 64, 64, seed=F.SEED, frame=F.FRAME0)
        assert abs(float(d.astype(np.float64).mean())) < 0.02 and 0.27 < float(d.std()) < 0.31          # uniform: 1 / sqrt(12) = 0.289
        for t in (100.0, 100.25, 100.5, 100.75, 100.9, 16.1, 234.6):
            mean = F.quantise(np.full((64, 64), t, f32), d, 0, 255).mean()
            assert abs(mean - t) <= 0.04, (comp, t, mean)


def test_random_pattern_changes_with_frame_component_and_seed():
    a = F.d_plane("random", 0, 16, 32, seed=F.SEED, frame=0)
    assert (a != F.d_plane("random", 0, 16, 32, seed=F.SEED, frame=1)).mean() > 0.4
    assert (a != F.d_plane("random", 1, 16, 32, seed=F.SEED, frame=0)).mean() > 0.4
    assert (a != F.d_plane("random", 2, 16, 32, seed=F.SEED, frame=0)).mean() > 0.4
    assert (a != F.d_plane("random", 0, 16, 32, seed=F.SEED + 1, frame=0)).mean() > 0.4
    assert (a != a.T[:16, :16].repeat(2, axis=1)).mean() > 0.4                     # rows and columns are not interchangeable
    assert np.array_equal(a, F.d_plane("random", 0, 16, 32, seed=F.SEED, frame=0))
    # ordered: static over frames
    assert np.array_equal(F.d_planes("ordered", 1, 3, 8, 8, frame0=0), F.d_planes("ordered", 1, 3, 8, 8, frame0=9))
    # frames beyond 2^32 still have keys of their own
    assert len({F.frame_key(1, f, c) for f in (0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40) for c in range(3)}) == 15


def test_none_is_the_existing_encoder():
    y = F.values(16, 24)
    want, _ = F.yuv_codes(y[..., :10, :22], "yuv420p", mode=None)
    plain = S.encode(y[..., :10, :22], "yuv420p", dtype=np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(want, plain))
    F.rgb_to_surface(y, "bgra", crop_to=(10, 22), mode=None)                         # asserts equality with rgb_surface_model.encode inside


# ---- the mutants the device comparison must catch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ordered", "random"])
@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv422p10le", "uyvy422", "nv12"])
def test_mutant_chroma_on_the_luma_grid_fails_the_device_inputs(pix_fmt, mode):
    for (H, W), (Hp, Wp) in F.PICTURES:
        rgb = F.values(Hp, Wp)[..., :H, :W]
        codes = F.yuv420_codes if pix_fmt == "nv12" else F.yuv_codes
        want, ties = codes(rgb, pix_fmt, mode=mode, seed=F.SEED, frame0=F.FRAME0)
        mutant, _ = codes(rgb, pix_fmt, mode=mode, seed=F.SEED, frame0=F.FRAME0, luma_grid_chroma=True)
        assert F.mismatches(want, want, ties) == 0
        assert F.mismatches(mutant, want, ties) > 0.1 * want[1].size, (pix_fmt, mode, H, W)
        assert np.array_equal(mutant[0], want[0])                                    # luma is on its own grid either way


@pytest.mark.parametrize("name", ["yuv444p", "bgra", "x2rgb10le"])
def test_mutant_call_local_frame_index_fails_the_device_inputs(name):
    (H, W), (Hp, Wp) = F.PICTURES[0]
    y = F.values(Hp, Wp)
    if name in S.FORMATS:
        want, ties = F.yuv_codes(y[..., :H, :W], name, mode="random", seed=F.SEED, frame0=F.FRAME0)
        mutant, _ = F.yuv_codes(y[..., :H, :W], name, mode="random", seed=F.SEED, frame0=F.FRAME0, local_index=True)
        assert F.mismatches(mutant, want, ties) > 0.1 * want[0].size
        # ... and one call of T frames is T calls of one frame with frame0 counted up, in the model as on the device
        for t in range(F.T):
            one, _ = F.yuv_codes(y[t:t + 1, :, :H, :W], name, mode="random", seed=F.SEED, frame0=F.FRAME0 + t)
            assert all(np.array_equal(o[0], w[t]) for o, w in zip(one, want))
    else:
        want = F.rgb_to_surface(y, name, crop_to=(H, W), mode="random", seed=F.SEED, frame0=F.FRAME0)
        mutant = F.rgb_to_surface(y, name, crop_to=(H, W), mode="random", seed=F.SEED, frame0=F.FRAME0, local_index=True)
        assert (want != mutant).mean() > 0.1
        for t in range(F.T):
            one = F.rgb_to_surface(y[t:t + 1], name, crop_to=(H, W), mode="random", seed=F.SEED, frame0=F.FRAME0 + t)
            assert np.array_equal(one[0], want[t])


# ---- the source ring ---------------------------------------------------------------------------------------------------------------------------
def test_source_ring_bookkeeping():
    torch = pytest.importorskip("torch")
    from bsvd_amd.pipeline import _SourceRing
    ring = _SourceRing(5, 4, 8, "cpu")
    assert ring.buf.shape == (5, 1, 3, 4, 8) and ring.buf.dtype == torch.float32
    with pytest.raises(RuntimeError, match="comes out before it went in"):
        ring.next_out()
    latency = 3

    def run(n, cut_at=None):
        """n frames fed (a cut changes nothing in the ring: frames keep their order), frame k read ``latency`` feeds later, then the tail"""
        got = []
        for k in range(n):
            ring.next_in().fill_(float(k))
            if k >= latency:
                got.append(float(ring.next_out()[0, 0, 0, 0]))
        while ring.emitted < ring.fed:
            got.append(float(ring.next_out()[0, 0, 0, 0]))
        return got
    assert run(13, cut_at=6) == [float(k) for k in range(13)]                     # more than two turns of the ring, in order
    with pytest.raises(RuntimeError, match="frame 13 comes out before it went in"):
        ring.next_out()
    ring.reset()                                                                  # flush(): the next stream starts at slot 0 again
    assert (ring.fed, ring.emitted) == (0, 0)
    assert run(7) == [float(k) for k in range(7)]
    assert ring.next_in().data_ptr() == ring.buf[7 % 5].data_ptr()                # nothing allocated: views of the one buffer


def test_finish_arguments_are_checked_without_a_device():
    from bsvd_amd import frame_io
    from bsvd_amd.pipeline import Colour, _Finish, _pixel_format
    assert frame_io.check_strength(0.7) == (0.7, 0.7) and frame_io.check_strength((0.4, 1)) == (0.4, 1.0)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x", (0.5,), (0.5, 0.5, 0.5), (0.5, 2.0), None):
        with pytest.raises(ValueError, match="strength"):
            frame_io.check_strength(bad)
    assert frame_io.check_dither(None) == (0, 0, 0) and frame_io.check_dither("random", 7, 5) == (2, 7, 5)
    for kw in (dict(dither="bayer"), dict(dither=1), dict(dither="ordered", dither_seed=-1), dict(dither="ordered", dither_seed=2 ** 32),
               dict(dither="random", frame0=-1), dict(dither="random", dither_seed="x")):
        with pytest.raises(ValueError, match="dither|frame0"):
            frame_io.check_dither(**kw)
    for bad in ("bt470", (0.5, 0.5), (0.2, 0.7, 1.1)):
        with pytest.raises(ValueError, match="matrix"):
            frame_io._luma_weights(bad)
    f = _Finish(_pixel_format("nv12", Colour(matrix="bt601")), 1.0, None, 0, None)
    assert not f.blends and f.dither_kw(3) == {} and f.matrix == "bt601"
    f = _Finish(_pixel_format("bgra", None), (0.4, 1.0), "random", 9, None)
    assert f.blends and f.matrix == "bt709"
    assert f.dither_kw(3) == dict(dither="random", dither_seed=9, frame0=0) and f.dither_kw(1)["frame0"] == 3
    assert _Finish(_pixel_format("bgra", None), 0.5, None, 0, "bt2020").matrix == "bt2020"


# ---- the ABI's refusals ------------------------------------------------------------------------------------------------------------------------
def _load():
    from bsvd_amd import _lib
    return _lib, _lib.load()


def test_new_entry_points_are_exported():
    _lib, lib = _load()
    for name in ("bsvd_blend_planar", "bsvd_planar_to_yuv420_crop_d", "bsvd_planar_to_yuv_crop_d", "bsvd_planar_to_rgb_d"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.BsvdDither) == 24 and _lib.ABI_VERSION == 12
    assert _lib.DITHER == {None: F.NONE, "ordered": F.ORDERED, "random": F.RANDOM}
    for name, w in F.LUMA_W.items():
        assert _lib.LUMA_WEIGHTS[name] == w


def test_blend_refusals_name_the_argument():
    _lib, lib = _load()
    w = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    P = 4096                                                            # a pointer value: every case below is refused before it is used
    good = dict(y=P, y_fs=3 * 16 * 32, x=P * 2, x_fs=4 * 16 * 32, frames=2, Hp=16, Wp=32, s_l=0.5, s_c=0.5, w=w)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bsvd_blend_planar(a["y"], a["y_fs"], a["x"], a["x_fs"], a["frames"], a["Hp"], a["Wp"], a["s_l"], a["s_c"], a["w"], None)
        return rc, lib.bsvd_last_error().decode()

    cases = [(dict(y=None), "y is NULL"), (dict(x=None), "x is NULL"), (dict(w=None), "luma_w is NULL"),
             (dict(frames=0), "frames = 0"), (dict(frames=-1), "frames = -1"), (dict(Hp=0), "Hp = 0"), (dict(Wp=-4), "Wp = -4"),
             (dict(y_fs=3 * 16 * 32 - 1), "y_frame_stride = 1535"), (dict(x_fs=2 * 16 * 32), "x_frame_stride = 1024"),
             (dict(s_l=-0.01), "s_luma"), (dict(s_l=1.01), "s_luma"), (dict(s_l=float("nan")), "s_luma"), (dict(s_l=float("inf")), "s_luma"),
             (dict(s_c=-0.01), "s_chroma"), (dict(s_c=1.5), "s_chroma"), (dict(s_c=float("nan")), "s_chroma"), (dict(s_c=float("-inf")), "s_chroma"),
             (dict(y=P + 2), "y must be 4-byte aligned"), (dict(x=2 * P + 1), "x must be 4-byte aligned"),
             (dict(w=(ctypes.c_float * 3)(0.2, float("nan"), 0.1)), "luma_w[1]")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -3 and err.startswith("bsvd_blend_planar: ") and text in err, (kw, rc, err)


def test_dithered_encoders_refuse_what_the_plain_ones_refuse_and_a_bad_dither():
    _lib, lib = _load()
    P = 4096
    desc = _lib.BsvdYuvDesc(pix_fmt=0, matrix=1, full_range=0, chroma=1)
    sub, layout, bits, high = _lib.YUV_FORMATS["yuv422p"]
    surf = _lib.BsvdYuvSurface(subsampling=sub, layout=layout, bits=bits, high_bits=high, matrix=1, chroma=1)
    lay, comp, rbits, pos, fourth = _lib.RGB_FORMATS["bgra"]
    rgb = _lib.BsvdRgbSurface(layout=lay, components=comp, bits=rbits, fourth=fourth, full_range=1)
    rgb.pos[:] = pos

    def refused(dither, text, **kw):
        # (each call's message is read right behind it)
        d = None if dither is None else ctypes.byref(dither)
        src = kw.get("src", P)
        H = kw.get("H", 10)
        for fn, args in (("bsvd_planar_to_yuv420_crop_d", (ctypes.byref(desc), d, None)), ("bsvd_planar_to_yuv_crop_d", (ctypes.byref(surf), d, None)),
                         ("bsvd_planar_to_rgb_d", (ctypes.byref(rgb), None, d, None))):
            rc = getattr(lib, fn)(src, 2 * P, 2, 16, 24, H, 22, *args)
            err = lib.bsvd_last_error().decode()
            assert rc == -3 and err.startswith(fn + ": ") and text in err, (fn, rc, err)

    refused(None, "dither is NULL")
    refused(_lib.BsvdDither(mode=3), "dither->mode = 3")
    refused(_lib.BsvdDither(mode=-1), "dither->mode = -1")
    refused(_lib.BsvdDither(mode=2, frame0=-1), "dither->frame0 = -1")
    refused(_lib.BsvdDither(mode=1, reserved=1), "dither->reserved = 1")
    refused(_lib.BsvdDither(mode=1), "src is NULL", src=None)                       # the plain entry points' refusals, under the new names
    refused(_lib.BsvdDither(mode=1), "H = 0", H=0)
