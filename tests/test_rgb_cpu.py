"""RGB surfaces without a GPU (include/bsvd_hip.h, BsvdRgbSurface): the numpy model of tests/rgb_surface_model.py against an independent
per-pixel statement of every format, the round trips of the code arithmetic, bsvd_rgb_frame_bytes and every refusal of the two entry points
(validation needs no device), the Python argument errors, and LiveStream's alpha ring driven with a stub model and stub kernels."""
import contextlib
import ctypes
import struct
import types

import numpy as np
import pytest
import torch

import rgb_surface_model as R

NAMES = sorted(R.FORMATS)
# what ffmpeg's pixel format descriptions say, written out by hand: (samples of a pixel in memory order | fields of the word from the msb |
# planes), bits.  Independent of R.FORMATS' order strings on purpose.
FFMPEG = {
    "rgb24": ("packed", ["R", "G", "B"], 8), "bgr24": ("packed", ["B", "G", "R"], 8),
    "rgba": ("packed", ["R", "G", "B", "A"], 8), "bgra": ("packed", ["B", "G", "R", "A"], 8),
    "argb": ("packed", ["A", "R", "G", "B"], 8), "abgr": ("packed", ["A", "B", "G", "R"], 8),
    "rgb0": ("packed", ["R", "G", "B", "X"], 8), "bgr0": ("packed", ["B", "G", "R", "X"], 8),
    "0rgb": ("packed", ["X", "R", "G", "B"], 8), "0bgr": ("packed", ["X", "B", "G", "R"], 8),
    "rgb48le": ("packed", ["R", "G", "B"], 16), "bgr48le": ("packed", ["B", "G", "R"], 16),
    "rgba64le": ("packed", ["R", "G", "B", "A"], 16), "bgra64le": ("packed", ["B", "G", "R", "A"], 16),
    "x2rgb10le": ("word", ["R", "G", "B"], 10), "x2bgr10le": ("word", ["B", "G", "R"], 10),
    "gbrp": ("planar", ["G", "B", "R"], 8), "gbrp10le": ("planar", ["G", "B", "R"], 10), "gbrp12le": ("planar", ["G", "B", "R"], 12),
    "gbrp16le": ("planar", ["G", "B", "R"], 16),
    "gbrap": ("planar", ["G", "B", "R", "A"], 8), "gbrap10le": ("planar", ["G", "B", "R", "A"], 10), "gbrap12le": ("planar", ["G", "B", "R", "A"], 12),
    "gbrap16le": ("planar", ["G", "B", "R", "A"], 16),
}


def _codes(rng, bits, shape):
    return rng.randint(0, 1 << bits, shape).astype(np.int64)


def _by_hand(px, name, H, W):
    """px[y][x] = {'R':, 'G':, 'B':, 'A' / 'X':} -> the tight frame's bytes, pixel by pixel"""
    kind, order, bits = FFMPEG[name]
    out = bytearray()
    if kind == "word":
        for y in range(H):
            for x in range(W):
                p = px[y][x]
                out += struct.pack("<I", (p[order[0]] << 20) | (p[order[1]] << 10) | p[order[2]])
    elif kind == "packed":
        for y in range(H):
            for x in range(W):
                for c in order:
                    out += struct.pack("<B" if bits == 8 else "<H", px[y][x][c])
    else:
        for c in order:
            for y in range(H):
                for x in range(W):
                    out += struct.pack("<B" if bits == 8 else "<H", px[y][x][c])
    return bytes(out)


def test_names():
    from bsvd_amd import _lib
    assert sorted(_lib.RGB_FORMATS) == NAMES == sorted(FFMPEG) and len(NAMES) == 24


@pytest.mark.parametrize("name", NAMES)
def test_model_against_a_per_pixel_statement(name):
    H, W = 3, 5
    rng = np.random.RandomState(NAMES.index(name))
    bits = FFMPEG[name][2]
    r, g, b, f = (_codes(rng, bits, (1, H, W)) for _ in range(4))
    px = [[{"R": int(r[0, y, x]), "G": int(g[0, y, x]), "B": int(b[0, y, x]), "A": int(f[0, y, x]), "X": int(f[0, y, x])} for x in range(W)]
          for y in range(H)]
    want = _by_hand(px, name, H, W)
    buf = R.pack(r, g, b, name, f)
    assert buf.shape == (1, len(want)) == (1, R.frame_bytes(H, W, name)) and buf.tobytes() == want
    r2, g2, b2, f2, ignored = R.unpack(np.frombuffer(want, np.uint8).reshape(1, -1), H, W, name)
    assert np.array_equal(r2, r) and np.array_equal(g2, g) and np.array_equal(b2, b) and ignored == 0
    if len(FFMPEG[name][1]) == 4:
        assert np.array_equal(f2, f)
    else:
        assert f2 is None
    # the bits a reader ignores: set to ones, and still the same codes
    junk = R.pack(r, g, b, name, f, junk="ones")
    r3, g3, b3, f3, ignored = R.unpack(junk, H, W, name)
    assert np.array_equal(r3, r) and np.array_equal(g3, g) and np.array_equal(b3, b)
    assert (ignored != 0) == (bits in (10, 12))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_every_code_round_trips(bits):
    codes = np.arange(1 << bits, dtype=np.int64)
    assert np.array_equal(R.encode(R.decode(codes, bits, True), bits, True), codes)
    s = 1 << (bits - 8)
    back = R.encode(R.decode(codes, bits, False), bits, False)
    assert np.array_equal(back, np.clip(codes, 16 * s, 235 * s))          # legal codes come back, illegal ones land on the nearest legal end
    v = R.decode(codes, bits, False)
    assert v.dtype == np.float32 and v[0] < 0 and v[-1] > 1              # the decode does not clamp


def test_rgb24_is_the_u8_pair():
    """the model at 8 bits full range is the numpy statement of bsvd_u8_to_planar / bsvd_planar_to_u8: code / 255; clamp, x 255, rint"""
    rng = np.random.RandomState(5)
    px = rng.randint(0, 256, (2, 4, 8, 3)).astype(np.uint8)
    for name, view in (("rgb24", px), ("bgr24", px[..., ::-1])):
        x, alpha = R.to_input(np.ascontiguousarray(view).reshape(2, -1), 4, 8, name)
        assert alpha is None and x.dtype == np.float32
        assert np.array_equal(x, px.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255))
    y = (rng.rand(2, 3, 4, 8) * 1.4 - 0.2).astype(np.float32)
    want = np.rint(np.clip(y, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(R.to_surface(y, "rgb24").reshape(2, 4, 8, 3), want)
    assert np.array_equal(R.to_surface(y, "bgr24").reshape(2, 4, 8, 3), want[..., ::-1])


def test_model_filler_alpha_and_x_bits():
    y = np.full((1, 3, 2, 4), 0.5, np.float32)
    a = np.arange(8).reshape(1, 2, 4)
    assert set(R.unpack(R.to_surface(y, "bgr0"), 2, 4, "bgr0")[3].ravel()) == {255}
    assert set(R.unpack(R.to_surface(y, "rgba64le"), 2, 4, "rgba64le")[3].ravel()) == {65535}
    assert np.array_equal(R.unpack(R.to_surface(y, "gbrap12le", alpha=a), 2, 4, "gbrap12le")[3], a)
    assert R.unpack(R.to_surface(y, "x2rgb10le"), 2, 4, "x2rgb10le")[4] == 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the library without a device

def _surface(name, **over):
    from bsvd_amd import _lib
    layout, components, bits, pos, fourth = _lib.RGB_FORMATS[name]
    s = _lib.BsvdRgbSurface(layout=layout, components=components, bits=bits, fourth=fourth, full_range=1)
    s.pos[:] = pos
    for k, v in over.items():
        if k in ("pitch", "offset", "pos"):
            getattr(s, k)[:] = tuple(v) + (0,) * (4 - len(v))
        else:
            setattr(s, k, v)
    return s


def test_struct_and_abi():
    from bsvd_amd import _lib
    lib = _lib.load()
    S = _lib.BsvdRgbSurface
    assert ctypes.sizeof(S) == 104
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == {"layout": 0, "components": 4, "bits": 8, "pos": 12, "fourth": 28, "full_range": 32,
                                                                "pitch": 36, "reserved0": 52, "offset": 56, "frame_stride": 88, "reserved": 96}
    assert _lib.ABI_VERSION == 12 and lib.bsvd_abi_version() == 12
    assert ctypes.sizeof(_lib.BsvdConvArgs) == 272 == lib.bsvd_conv_args_size()
    for name in ("bsvd_rgb_frame_bytes", "bsvd_rgb_to_planar", "bsvd_planar_to_rgb"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("name", NAMES)
def test_frame_bytes_against_the_model(name):
    from bsvd_amd.frame_io import rgb_frame_bytes
    sb = R.sample_bytes(name)
    for H, W in ((4, 8), (5, 7), (1, 1), (3, 130)):
        assert rgb_frame_bytes(H, W, name) == R.frame_bytes(H, W, name), (H, W)
        n = len(R.planes(H, W, name))
        row = R.planes(H, W, name)[0][1]
        pitches = [row + 4 * (i + 1) for i in range(n)]
        assert rgb_frame_bytes(H, W, name, pitches) == R.frame_bytes(H, W, name, pitches)
        offsets = [8 + i * (pitches[i] * H + 12) for i in range(n)]
        assert rgb_frame_bytes(H, W, name, pitches, offsets) == R.frame_bytes(H, W, name, pitches, offsets) == offsets[-1] + pitches[-1] * H
    assert sb in (1, 2, 4)


def _call_both(a):
    from bsvd_amd import _lib
    lib = _lib.load()
    out = []
    rc = lib.bsvd_rgb_to_planar(a["rgb"], a["planar"], a["frames"], a["H"], a["W"], a["Hp"], a["Wp"], a["surface"], a["alpha"], a["cc"], 0.1, None)
    out.append(("bsvd_rgb_to_planar", rc, lib.bsvd_last_error().decode()))
    rc = lib.bsvd_planar_to_rgb(a["planar"], a["rgb"], a["frames"], a["Hp"], a["Wp"], a["H"], a["W"], a["surface"], a["alpha"], None)
    out.append(("bsvd_planar_to_rgb", rc, lib.bsvd_last_error().decode()))
    return out


# (format, changes to a valid 8 x 12 call, the words the error must contain): every case of the header's list
BAD = [
    ("bgra", dict(rgb=None), "is NULL"), ("bgra", dict(planar=None), "is NULL"), ("bgra", dict(surface=None), "surface is NULL"),
    ("rgb24", dict(frames=0), "frames"), ("rgb24", dict(frames=-1), "frames"),
    ("rgb24", dict(H=0), "H = 0"), ("rgb24", dict(W=-4), "W = -4"),
    ("rgb24", dict(Hp=7), "Hp = 7"), ("rgb24", dict(Wp=11), "Wp = 11"),
    ("rgb24", dict(H=4, Hp=8), "Hp = 8"), ("rgb24", dict(W=6, Wp=12), "Wp = 12"),        # a pad of a whole dimension
    ("gbrp", dict(s=dict(layout=3)), "layout"), ("gbrp", dict(s=dict(layout=-1)), "layout"),
    ("rgb24", dict(s=dict(components=2)), "components"), ("rgb24", dict(s=dict(components=5)), "components"),
    ("x2rgb10le", dict(s=dict(components=4, fourth=1, pos=(0, 1, 2, 3))), "components"),
    ("rgb24", dict(s=dict(bits=9)), "bits"), ("gbrp", dict(s=dict(bits=14)), "bits"), ("rgb48le", dict(s=dict(bits=32)), "bits"),
    ("x2rgb10le", dict(s=dict(bits=8)), "bits"), ("x2bgr10le", dict(s=dict(bits=12)), "bits"),
    ("rgba", dict(s=dict(fourth=3)), "fourth"), ("rgba", dict(s=dict(fourth=0)), "fourth"), ("rgb24", dict(s=dict(fourth=1)), "fourth"),
    ("gbrp", dict(s=dict(fourth=2)), "fourth"),
    ("bgra", dict(s=dict(full_range=2)), "full_range"), ("bgra", dict(s=dict(full_range=-1)), "full_range"),
    ("rgb24", dict(s=dict(pos=(0, 0, 1))), "pos"), ("rgb24", dict(s=dict(pos=(0, 1, 3))), "pos"), ("rgb24", dict(s=dict(pos=(0, 1, 2, 3))), "pos[3]"),
    ("bgra", dict(s=dict(pos=(0, 1, 2, 2))), "pos"), ("gbrap", dict(s=dict(pos=(-1, 0, 1, 2))), "pos"),
    ("x2rgb10le", dict(s=dict(pos=(1, 1, 0))), "pos"),
    ("bgra", dict(s=dict(reserved0=1)), "reserved0"), ("bgra", dict(s=dict(reserved=1)), "reserved"),
    ("rgb24", dict(s=dict(pitch=(35,))), "pitch[0]"),                                      # 12 pixels are 36 bytes
    ("bgra", dict(s=dict(pitch=(47,))), "pitch[0]"), ("rgb48le", dict(s=dict(pitch=(70,))), "pitch[0]"),
    ("rgb48le", dict(s=dict(pitch=(73,))), "pitch[0]"),                                    # odd with 16-bit samples
    ("x2rgb10le", dict(s=dict(pitch=(50,))), "pitch[0]"),                                  # words want 4
    ("gbrp", dict(s=dict(pitch=(0, 11, 0))), "pitch[1]"), ("gbrap10le", dict(s=dict(pitch=(0, 0, 0, 25))), "pitch[3]"),
    ("rgb24", dict(s=dict(pitch=(0, 40))), "pitch[1]"), ("gbrp", dict(s=dict(pitch=(0, 0, 0, 16))), "pitch[3]"),      # planes the layout lacks
    ("bgra", dict(s=dict(offset=(0, 64))), "offset[1]"), ("gbrp", dict(s=dict(offset=(0, 0, 0, 512))), "offset[3]"),
    ("rgb24", dict(s=dict(offset=(-1,))), "offset[0]"), ("gbrp", dict(s=dict(offset=(0, -96, 0))), "offset[1]"),
    ("rgb48le", dict(s=dict(offset=(1,))), "offset[0]"), ("x2rgb10le", dict(s=dict(offset=(2,))), "offset[0]"),
    ("gbrp16le", dict(s=dict(offset=(0, 0, 1001))), "offset[2]"),
    ("gbrp", dict(s=dict(offset=(0, 95, 0))), "share bytes"),                              # a plane is 96 bytes
    ("gbrap", dict(s=dict(offset=(0, 96, 192, 100))), "share bytes"),
    ("gbrp", dict(s=dict(offset=(200, 96, 150))), "share bytes"),
    ("rgb24", dict(s=dict(frame_stride=287)), "frame_stride"),                             # one tight 8 x 12 frame is 288 bytes
    ("bgra", dict(s=dict(pitch=(64,), frame_stride=384)), "frame_stride"),
    ("gbrp", dict(s=dict(offset=(16,), frame_stride=288)), "frame_stride"),
    ("rgb48le", dict(s=dict(frame_stride=577)), "frame_stride"), ("x2bgr10le", dict(s=dict(frame_stride=386)), "frame_stride"),
    ("rgb48le", dict(rgb=4097), "2-byte aligned"), ("gbrp10le", dict(rgb=4097), "2-byte aligned"), ("x2rgb10le", dict(rgb=4098), "4-byte aligned"),
    ("rgb24", dict(planar=8194), "4-byte aligned"),
    ("rgb24", dict(alpha=12288), "without alpha"), ("bgr0", dict(alpha=12288), "without alpha"), ("x2rgb10le", dict(alpha=12288), "without alpha"),
    ("gbrp12le", dict(alpha=12288), "without alpha"),
    ("rgba64le", dict(alpha=12289), "2-byte aligned"),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_refusals_name_their_argument(case):
    name, change, words = BAD[case]
    change = dict(change)
    s = _surface(name, **change.pop("s", {}))
    a = dict(rgb=4096, planar=8192, frames=2, H=8, W=12, Hp=8, Wp=12, surface=ctypes.byref(s), alpha=None, cc=1)
    a.update(change)
    for fn, rc, err in _call_both(a):
        assert rc == -3, (fn, rc, err)
        assert err.startswith(fn + ":") and words in err, (fn, err)


def test_const_channels_and_frame_bytes_refusals():
    from bsvd_amd import _lib
    lib = _lib.load()
    s = _surface("bgra")
    assert lib.bsvd_rgb_to_planar(4096, 8192, 1, 8, 12, 8, 12, ctypes.byref(s), None, -1, 0.0, None) == -3
    assert "const_channels" in lib.bsvd_last_error().decode()
    assert lib.bsvd_rgb_frame_bytes(8, 12, None) == -1 and lib.bsvd_rgb_frame_bytes(0, 12, ctypes.byref(s)) == -1
    assert lib.bsvd_rgb_frame_bytes(8, 12, ctypes.byref(_surface("bgra", pitch=(40,)))) == -1
    assert lib.bsvd_rgb_frame_bytes(8, 12, ctypes.byref(s)) == 8 * 12 * 4


def test_python_argument_errors():
    from bsvd_amd import frame_io
    from bsvd_amd.pipeline import ClipPipeline, LiveStream, _pixel_format
    for fn in (lambda: frame_io.rgb_frame_bytes(4, 4, "rgb32"), lambda: frame_io.rgb_to_input(None, 4, 4, "gray"),
               lambda: frame_io.output_to_rgb(None, "yuv420p")):
        with pytest.raises(ValueError, match="pix_fmt"):
            fn()
    with pytest.raises(ValueError, match="multiples of 4"):
        frame_io.rgb_to_input(torch.zeros(1, 5 * 7 * 4, dtype=torch.uint8), 5, 7, "bgra")
    with pytest.raises(ValueError, match="alpha"):
        frame_io.output_to_rgb(torch.zeros(1, 3, 4, 4), "bgr0", alpha=torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="alpha"):
        frame_io.rgb_to_input(torch.zeros(1, 48, dtype=torch.uint8), 4, 4, "rgb24", return_alpha=True)
    with pytest.raises(ValueError, match="pitches"):
        frame_io.rgb_frame_bytes(4, 4, "bgra", pitches=[16, 16])
    with pytest.raises(ValueError, match="sigma"):
        frame_io.rgb_to_input(torch.zeros(1, 64, dtype=torch.uint8), 4, 4, "bgra", sigma="soon")
    for colour in ({"matrix": "bt709"}, {"full_range": True, "chroma": "linear"}, ("bt709",)):
        with pytest.raises(ValueError, match="colour"):
            _pixel_format("bgra", colour)
    assert _pixel_format("bgra", None).full_range is True and _pixel_format("bgra", {"full_range": False}).full_range is False
    with pytest.raises(ValueError, match="frame_shape"):
        _pixel_format("gbrp10le", None, frame_shape=5)
    with pytest.raises(ValueError, match="frame_shape"):
        _pixel_format("gbrp10le", None).geometry(np.zeros(48, np.uint16), clip=False)
    with pytest.raises(ValueError, match="multiples of 4"):
        _pixel_format("bgra", None, frame_shape=(5, 7))
    _pixel_format("bgra", None, pad="reflect", frame_shape=(5, 7))
    f = _pixel_format("bgra", None)
    for bad in (np.zeros((4, 8, 3), np.uint8), np.zeros((4, 8, 4), np.uint16), np.zeros((4, 4, 8), np.uint8)):
        with pytest.raises(ValueError, match="bgra"):
            f.geometry(bad, clip=False)
    g = f.geometry(np.zeros((4, 8, 4), np.uint8), clip=False)
    assert (g.h, g.w, g.staging, g.net_h, g.net_w) == (4, 8, (128,), 4, 8)
    assert _pixel_format("x2rgb10le", None).geometry(np.zeros((2, 4, 8), np.uint32), clip=True).staging == (2, 128)
    assert _pixel_format("gbrap16le", None).geometry(np.zeros((4, 4, 8), np.uint16), clip=False).staging == (256,)
    assert _pixel_format("rgb48le", None, frame_shape=(4, 8)).geometry(np.zeros(96, np.uint16), clip=False).staging == (192,)
    # before any device is asked for
    for cls in (ClipPipeline, LiveStream):
        with pytest.raises(ValueError, match="colour"):
            cls(None, pix_fmt="rgba64le", colour={"matrix": "bt601"})
        with pytest.raises(ValueError, match="pix_fmt"):
            cls(None, pix_fmt="rgb32")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# LiveStream's alpha ring with a stub model and stub kernels: alpha k comes back with frame k

class _StubModel:
    """the streaming API's timing: frame k comes out ``latency`` feeds after it went in; None feeds drain"""
    shift_num = 16

    def __init__(self, overlap):
        self.overlap, self.q, self.cuts = overlap, [], []
        self.net = types.SimpleNamespace(net_in_ch=3)

    def _device(self):
        return types.SimpleNamespace(type="cuda")

    def reset(self):
        self.q = []

    def overlap_available(self, shape):
        return self.overlap

    def _feed(self, x, latency, cut):
        if x is not None:
            self.q.append(x)
            self.cuts.append(bool(cut))
        return self.q.pop(0) if self.q and (x is None or len(self.q) > latency) else None

    def feedin_one_element(self, x, cut=False):
        return self._feed(x, 16, cut)

    def feed_overlapped(self, x, last=False, cut=False):
        return self._feed(x, 17, cut)


class _Quiet:
    def __init__(self, *a, **k):
        pass

    def record(self):
        pass

    def synchronize(self):
        pass

    def wait_event(self, e):
        pass


def _stub_device(monkeypatch):
    """the stream plumbing of the pipelines as no-ops, and the two conversion kernels as the numpy model on host tensors"""
    from bsvd_amd import pipeline
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Stream", _Quiet)
    monkeypatch.setattr(torch.cuda, "Event", _Quiet)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda t: t)

    def to_input(buf, H, W, pix_fmt, full_range=True, sigma=None, sigma_gain=1.0, pad_to=None, return_alpha=False):
        x, alpha = R.to_input(buf.numpy(), H, W, pix_fmt, full_range, pad_to=pad_to)
        return_alpha.copy_(torch.from_numpy(alpha))
        return torch.from_numpy(x), return_alpha

    def to_output(y, pix_fmt, full_range=True, crop_to=None, alpha=None):
        return torch.from_numpy(R.to_surface(y.numpy(), pix_fmt, full_range, crop_to=crop_to, alpha=alpha.numpy()))
    monkeypatch.setattr(pipeline, "rgb_to_input", to_input)
    monkeypatch.setattr(pipeline, "output_to_rgb", to_output)


@pytest.mark.parametrize("overlap,depth,size,pad", [(False, 1, (4, 8), None), (True, 2, (4, 8), None), (True, 3, (5, 7), "reflect")])
def test_alpha_comes_back_with_its_frame(monkeypatch, overlap, depth, size, pad):
    from bsvd_amd.pipeline import LiveStream
    _stub_device(monkeypatch)
    model = _StubModel(overlap)
    live = LiveStream(model, depth=depth, overlap_blocks=overlap, pix_fmt="bgra", pad=pad)
    live.device = torch.device("cpu")
    assert live.latency == 16 + depth - 1 + (1 if overlap else 0)
    H, W = size
    rng = np.random.RandomState(7)
    n = 2 * (live.latency + depth) + 5                                   # every ring plane is written at least twice
    frames = rng.randint(0, 256, (n, H, W, 4)).astype(np.uint8)
    got = []
    for k, f in enumerate(frames):
        r = live.feed(f, cut=(k == 20))
        assert (r is None) == (k < live.latency), k
        if r is not None:
            got.append(r)
    ring = live._alpha.buf
    assert ring.shape == (live.latency + depth, 1, H, W) and ring.dtype == torch.uint8
    got += live.flush()
    assert len(got) == n and model.cuts.count(True) == 1 and model.cuts[20]
    for k, r in enumerate(got):
        assert r.shape == (H, W, 4) and r.dtype == np.uint8
        assert np.array_equal(r[..., 3], frames[k][..., 3]), "frame %d came back with another frame's alpha" % k
        assert np.array_equal(r[..., :3], frames[k][..., :3]), k         # the stub network is the identity, and 8-bit codes round-trip
    # a second stream on the same object: the ring starts over, nothing is allocated anew
    more = [live.feed(f) for f in frames[:live.latency + 2]] + live.flush()
    more = [r for r in more if r is not None]
    assert live._alpha.buf is ring and len(more) == live.latency + 2
    assert all(np.array_equal(r, frames[k]) for k, r in enumerate(more))
