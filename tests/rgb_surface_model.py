"""The RGB surfaces in numpy, written from the text of include/bsvd_hip.h (BsvdRgbSurface, bsvd_rgb_to_planar / bsvd_planar_to_rgb) and
independent of the library and of bsvd_amd._lib's table: the test model of tests/test_rgb_cpu.py and tests/test_gpu_rgb.py.

A format is (layout, order, bits): layout 'packed' (order = the samples of a pixel in memory order), 'x2' (order = the three 10-bit fields
of the 32-bit little-endian word from the LEAST significant one) or 'planar' (order = the planes); order's letters are r, g, b, a (alpha)
and 0 (a filler).  Codes are integer arrays [T,H,W]; ``pack`` / ``unpack`` move them into and out of byte buffers with per-plane pitches
and offsets and a frame stride; ``decode`` / ``encode`` are the arithmetic in the dtype given (float32: the device's bits); ``to_input`` /
``to_surface`` are the two entry points whole, pad / crop, filler and alpha included."""
import collections

import numpy as np

Format = collections.namedtuple("Format", "layout order bits")
FORMATS = {
    "rgb24": Format("packed", "rgb", 8), "bgr24": Format("packed", "bgr", 8),
    "rgba": Format("packed", "rgba", 8), "bgra": Format("packed", "bgra", 8), "argb": Format("packed", "argb", 8), "abgr": Format("packed", "abgr", 8),
    "rgb0": Format("packed", "rgb0", 8), "bgr0": Format("packed", "bgr0", 8), "0rgb": Format("packed", "0rgb", 8), "0bgr": Format("packed", "0bgr", 8),
    "rgb48le": Format("packed", "rgb", 16), "bgr48le": Format("packed", "bgr", 16),
    "rgba64le": Format("packed", "rgba", 16), "bgra64le": Format("packed", "bgra", 16),
    "x2rgb10le": Format("x2", "bgr", 10), "x2bgr10le": Format("x2", "rgb", 10),       # (msb) X R G B (lsb): B is the lowest field
    "gbrp": Format("planar", "gbr", 8), "gbrp10le": Format("planar", "gbr", 10), "gbrp12le": Format("planar", "gbr", 12), "gbrp16le": Format("planar", "gbr", 16),
    "gbrap": Format("planar", "gbra", 8), "gbrap10le": Format("planar", "gbra", 10), "gbrap12le": Format("planar", "gbra", 12),
    "gbrap16le": Format("planar", "gbra", 16),
}


def has_alpha(name):
    return "a" in FORMATS[name].order


def has_filler(name):
    return "0" in FORMATS[name].order


def sample_bytes(name):
    f = FORMATS[name]
    return 4 if f.layout == "x2" else 1 if f.bits == 8 else 2


def container(name):
    """numpy dtype of a sample (and of the alpha side plane)"""
    return np.dtype({1: "u1", 2: "<u2", 4: "<u4"}[sample_bytes(name)])


def planes(H, W, name):
    """-> [(rows, row bytes)] of the format's planes"""
    f = FORMATS[name]
    if f.layout == "planar":
        return [(H, W * sample_bytes(name))] * len(f.order)
    return [(H, W * 4 if f.layout == "x2" else W * len(f.order) * sample_bytes(name))]


def geometry(H, W, name, pitches=None, offsets=None, frame_stride=None):
    """-> (pitches, offsets, frame bytes, frame stride), all resolved: pitch 0 / None = tight, offset 0 / None of a later plane = directly
    behind the plane before (its pitch times H), frame bytes = the end of the plane that ends last"""
    pl = planes(H, W, name)
    pitches = list(pitches or ()) + [0] * 4
    offsets = list(offsets or ()) + [0] * 4
    P, O, end = [], [], 0
    for i, (rows, rb) in enumerate(pl):
        P.append(pitches[i] or rb)
        O.append(offsets[i] if i == 0 or offsets[i] else O[i - 1] + P[i - 1] * rows)
        end = max(end, O[i] + P[i] * rows)
    return P, O, end, frame_stride or end


def frame_bytes(H, W, name, pitches=None, offsets=None):
    return geometry(H, W, name, pitches, offsets)[2]


def _ignored_bits(junk, nbits, shape):
    """what goes into the bits a reader must ignore: all ones (junk == 'ones') or random (a RandomState)"""
    return np.full(shape, (1 << nbits) - 1, np.int64) if isinstance(junk, str) else junk.randint(0, 1 << nbits, shape)


def _raw_planes(comp, name, junk, x_ones=False):
    """comp: {letter: codes [T,H,W]} -> the byte arrays [T, H, row bytes] of each plane.  junk (a RandomState): the bits a reader must
    ignore -- above `bits` in a 16-bit word, the two X bits -- are random, or with junk = 'ones' all ones, instead of zero"""
    f = FORMATS[name]
    T, H, W = comp[f.order[0]].shape
    if f.layout == "x2":
        w = sum(comp[c].astype(np.uint32) << np.uint32(10 * i) for i, c in enumerate(f.order))
        if junk is not None:
            w = w | (_ignored_bits(junk, 2, w.shape).astype(np.uint32) << np.uint32(30))
        if x_ones:
            w = w | np.uint32(3 << 30)
        return [np.ascontiguousarray(w.astype("<u4")).view(np.uint8).reshape(T, H, 4 * W)]
    dt = container(name)

    def raw(samples):                                   # [T,H,n] codes -> bytes
        s = samples.astype(np.uint16 if f.bits > 8 else np.uint8)
        if junk is not None and f.bits in (10, 12):
            s = s | (_ignored_bits(junk, 16 - f.bits, s.shape).astype(np.uint16) << np.uint16(f.bits))
        return np.ascontiguousarray(s.astype(dt)).view(np.uint8).reshape(T, H, -1)
    if f.layout == "planar":
        return [raw(comp[c]) for c in f.order]
    return [raw(np.stack([comp[c] for c in f.order], axis=-1).reshape(T, H, W * len(f.order)))]


def pack(R, G, B, name, fourth=None, pitches=None, offsets=None, frame_stride=None, fill=0, junk=None, x_ones=False):
    """codes [T,H,W] -> uint8 [T, frame_stride]; every byte that is not a sample is ``fill``.  fourth: the alpha / filler codes of a
    four-sample format; x_ones: the two unused bits of an x2 word are ones (what the encoder writes) instead of zeros"""
    f = FORMATS[name]
    T, H, W = R.shape
    comp = {"r": R, "g": G, "b": B, "a": fourth, "0": fourth}
    P, O, _, stride = geometry(H, W, name, pitches, offsets, frame_stride)
    buf = np.full((T, stride), fill, np.uint8)
    for raw, (rows, rb), pitch, off in zip(_raw_planes(comp, name, junk, x_ones), planes(H, W, name), P, O):
        for r in range(rows):
            buf[:, off + r * pitch:off + r * pitch + rb] = raw[:, r]
    return buf


def unpack(buf, H, W, name, pitches=None, offsets=None):
    """uint8 [T, >= frame bytes] -> (R, G, B, fourth or None, ignored): integer codes, and the OR of every ignored bit (shifted down)"""
    f = FORMATS[name]
    T = buf.shape[0]
    P, O, _, _ = geometry(H, W, name, pitches, offsets)
    got, ignored = [], 0
    for (rows, rb), pitch, off in zip(planes(H, W, name), P, O):
        raw = np.ascontiguousarray(np.stack([buf[:, off + r * pitch:off + r * pitch + rb] for r in range(rows)], axis=1))
        words = raw.view(container(name)).astype(np.int64)
        if f.layout == "x2":
            ignored |= int(np.bitwise_or.reduce((words >> 30).ravel()))
        else:
            ignored |= int(np.bitwise_or.reduce((words >> f.bits).ravel()))
            words = words & ((1 << f.bits) - 1)
        got.append(words)
    if f.layout == "planar":
        comp = dict(zip(f.order, got))
    elif f.layout == "x2":
        comp = {c: (got[0] >> (10 * i)) & 1023 for i, c in enumerate(f.order)}
    else:
        px = got[0].reshape(T, H, W, len(f.order))
        comp = {c: px[..., i] for i, c in enumerate(f.order)}
    return comp["r"], comp["g"], comp["b"], comp.get("a", comp.get("0")), ignored


def sample_mask(T, H, W, name, pitches=None, offsets=None, frame_stride=None):
    """bool [T, frame_stride]: True where a byte belongs to a sample"""
    z = np.zeros((T, H, W), np.int64)
    return pack(z, z, z, name, z, pitches, offsets, frame_stride, fill=1) == 0


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------------
def decode(code, bits, full_range=True, dtype=np.float32):
    """codes -> values, not clamped: (float)code / (2^bits - 1), or ((float)code - 16 s) / (219 s)"""
    t = np.dtype(dtype).type
    s = 1 << (bits - 8)
    c = code.astype(dtype)
    return (c - t(0)) / t((1 << bits) - 1) if full_range else (c - t(16 * s)) / t(219 * s)


def encode(v, bits, full_range=True, dtype=np.float32):
    """values -> codes: clamp [0,1], one multiplication, one addition, round half to even, clamp to the legal codes"""
    t = np.dtype(dtype).type
    s = 1 << (bits - 8)
    mul, add, hi = (t((1 << bits) - 1), t(0), (1 << bits) - 1) if full_range else (t(219 * s), t(16 * s), 235 * s)
    x = np.clip(np.where(np.isnan(v), t(0), v).astype(dtype), t(0), t(1))              # fmaxf(NaN, 0) = 0
    return np.clip(np.rint(x * mul + add), float(add), hi).astype(np.int64)


def reflect_pad(x, Hp, Wp):
    """[..., H, W] -> [..., Hp, Wp]: element (r, c) = x[refl_H(r), refl_W(c)], refl_N(i) = i below N, else 2 (N - 1) - i"""
    H, W = x.shape[-2:]
    rows = [r if r < H else 2 * (H - 1) - r for r in range(Hp)]
    cols = [c if c < W else 2 * (W - 1) - c for c in range(Wp)]
    return x[..., rows, :][..., cols]


def to_input(buf, H, W, name, full_range=True, pitches=None, offsets=None, pad_to=None, const=None, dtype=np.float32):
    """bsvd_rgb_to_planar: uint8 [T, stride] -> ([T,3(+1),Hp,Wp], the alpha codes [T,H,W] in the container type, or None)"""
    f = FORMATS[name]
    R, G, B, fourth, _ = unpack(buf, H, W, name, pitches, offsets)
    x = np.stack([decode(c, f.bits, full_range, dtype) for c in (R, G, B)], axis=1)
    if const is not None:
        x = np.concatenate([x, np.full((x.shape[0], 1, H, W), const, dtype)], axis=1)
    if pad_to is not None:
        x = reflect_pad(x, *pad_to)
    return np.ascontiguousarray(x), (fourth.astype(container(name)) if has_alpha(name) else None)


def to_surface(y, name, full_range=True, pitches=None, offsets=None, frame_stride=None, crop_to=None, alpha=None, fill=0, dtype=np.float32):
    """bsvd_planar_to_rgb: [T,3,Hp,Wp] -> uint8 [T, stride]; alpha: codes [T,H,W] (masked to bits) or None = the maximum code; a filler
    is all ones"""
    f = FORMATS[name]
    H, W = crop_to if crop_to is not None else y.shape[-2:]
    y = y[:, :, :H, :W]
    top = (1 << f.bits) - 1
    fourth = None
    if len(f.order) == 4:
        fourth = np.full((y.shape[0], H, W), top, np.int64) if alpha is None or has_filler(name) else alpha.astype(np.int64) & top
    R, G, B = (encode(y[:, c], f.bits, full_range, dtype) for c in range(3))
    return pack(R, G, B, name, fourth, pitches, offsets, frame_stride, fill=fill, x_ones=True)
