"""The planar, 4:2:2 and 4:4:4 YUV surfaces in numpy, written from the text of include/bsvd_hip.h (BsvdYuvSurface, bsvd_yuv_to_planar /
bsvd_planar_to_yuv) and independent of the library: the test model of tests/test_yuv_formats_cpu.py and tests/test_gpu_yuv_formats.py.
The matrix constants, the code scales and the 4:2:0 filters are those of tests/yuv_model.py; the 4:2:2 filters are written here from the
header's formulas.  ``dtype`` is the arithmetic's type: float64 for the truth, float32 for fp32 arithmetic in this order.  Planes are
arrays of integer codes: Y [T,H,W]; Cb, Cr [T,H/2,W/2] (4:2:0), [T,H,W/2] (4:2:2), [T,H,W] (4:4:4).  ``pack`` / ``unpack`` move them into
and out of byte buffers with per-plane pitches and offsets and a frame stride."""
import collections

import numpy as np

import yuv_model as M

Format = collections.namedtuple("Format", "sub layout bits high")
# ffmpeg's names.  layout: 'planar' (Y, Cb, Cr planes), 'semi' (Y plane + interleaved CbCr plane), 'uyvy' (Cb Y0 Cr Y1), 'yuyv' (Y0 Cb Y1 Cr).
# high: 10-bit code in the high bits of the little-endian word (P010 rule) instead of the low bits.
FORMATS = {
    "yuv420p": Format(420, "planar", 8, False), "yuv420p10le": Format(420, "planar", 10, False),
    "uyvy422": Format(422, "uyvy", 8, False), "yuyv422": Format(422, "yuyv", 8, False),
    "nv16": Format(422, "semi", 8, False), "p210le": Format(422, "semi", 10, True),
    "yuv422p": Format(422, "planar", 8, False), "yuv422p10le": Format(422, "planar", 10, False),
    "yuv444p": Format(444, "planar", 8, False), "yuv444p10le": Format(444, "planar", 10, False),
}


def chroma_shape(H, W, sub):
    return (H // 2 if sub == 420 else H, W if sub == 444 else W // 2)


def planes(H, W, pix_fmt):
    """-> [(rows, row bytes)] of the format's planes"""
    f = FORMATS[pix_fmt]
    sb = 2 if f.bits > 8 else 1
    ch, cw = chroma_shape(H, W, f.sub)
    if f.layout in ("uyvy", "yuyv"):
        return [(H, 2 * W)]
    if f.layout == "semi":
        return [(H, W * sb), (ch, 2 * cw * sb)]
    return [(H, W * sb), (ch, cw * sb), (ch, cw * sb)]


def geometry(H, W, pix_fmt, pitches=None, offsets=None, frame_stride=None):
    """-> (pitches, offsets, frame bytes, frame stride), all resolved: pitch 0 / None = tight, offset 0 / None of planes 1, 2 = directly
    behind the plane before, frame bytes = the end of the plane that ends last"""
    pl = planes(H, W, pix_fmt)
    pitches = list(pitches or ()) + [0] * 3
    offsets = list(offsets or ()) + [0] * 3
    P, O, end = [], [], 0
    for i, (rows, rb) in enumerate(pl):
        P.append(pitches[i] or rb)
        O.append(offsets[i] if i == 0 or offsets[i] else O[i - 1] + P[i - 1] * pl[i - 1][0])
        end = max(end, O[i] + P[i] * rows)
    return P, O, end, frame_stride or end


def frame_bytes(H, W, pix_fmt, pitches=None, offsets=None):
    return geometry(H, W, pix_fmt, pitches, offsets)[2]


def _sample_planes(Y, Cb, Cr, f):
    """codes -> the sample arrays [T, rows, samples per row] of each plane"""
    T, H, W = Y.shape
    if f.layout == "planar":
        return [Y, Cb, Cr]
    if f.layout == "semi":
        return [Y, np.stack([Cb, Cr], axis=-1).reshape(T, Cb.shape[1], 2 * Cb.shape[2])]
    y = Y.reshape(T, H, W // 2, 2)
    group = [Cb, y[..., 0], Cr, y[..., 1]] if f.layout == "uyvy" else [y[..., 0], Cb, y[..., 1], Cr]
    return [np.stack(group, axis=-1).reshape(T, H, 2 * W)]


def pack(Y, Cb, Cr, pix_fmt, pitches=None, offsets=None, frame_stride=None, fill=0, junk=None):
    """codes -> uint8 [T, frame_stride]; every byte that is not a sample is ``fill``.  10 bit: the 6 bits of a word a reader must ignore
    are zero, or random with ``junk`` (a RandomState)."""
    f = FORMATS[pix_fmt]
    T, H, W = Y.shape
    P, O, _, stride = geometry(H, W, pix_fmt, pitches, offsets, frame_stride)
    buf = np.full((T, stride), fill, np.uint8)
    for samples, (rows, rb), pitch, off in zip(_sample_planes(Y, Cb, Cr, f), planes(H, W, pix_fmt), P, O):
        if f.bits > 8:
            words = samples.astype(np.uint16) << (6 if f.high else 0)
            if junk is not None:
                words = words | (junk.randint(0, 64, samples.shape).astype(np.uint16) << (0 if f.high else 10))
            raw = np.ascontiguousarray(words.astype("<u2")).view(np.uint8).reshape(T, rows, rb)
        else:
            raw = samples.astype(np.uint8)
        for r in range(rows):
            buf[:, off + r * pitch:off + r * pitch + rb] = raw[:, r]
    return buf


def unpack(buf, H, W, pix_fmt, pitches=None, offsets=None):
    """uint8 [T, >= frame bytes] -> (Y, Cb, Cr, ignored): integer codes and, for 10 bit, the OR of the ignored 6 bits of every word (else 0)"""
    f = FORMATS[pix_fmt]
    T = buf.shape[0]
    P, O, _, _ = geometry(H, W, pix_fmt, pitches, offsets)
    ch, cw = chroma_shape(H, W, f.sub)
    got, ignored = [], 0
    for (rows, rb), pitch, off in zip(planes(H, W, pix_fmt), P, O):
        raw = np.stack([buf[:, off + r * pitch:off + r * pitch + rb] for r in range(rows)], axis=1)
        if f.bits > 8:
            words = np.ascontiguousarray(raw).view("<u2").astype(np.int64)
            ignored |= int(np.bitwise_or.reduce((words & 63 if f.high else words >> 10).ravel()))
            got.append(words >> 6 if f.high else words & 1023)
        else:
            got.append(raw.astype(np.int64))
    if f.layout == "planar":
        Y, Cb, Cr = got
    elif f.layout == "semi":
        Y, c = got[0], got[1].reshape(T, ch, cw, 2)
        Cb, Cr = c[..., 0], c[..., 1]
    else:
        g = got[0].reshape(T, H, W // 2, 4)
        iy, ib, ir = ((1, 3), 0, 2) if f.layout == "uyvy" else ((0, 2), 1, 3)
        Y = np.stack([g[..., iy[0]], g[..., iy[1]]], axis=-1).reshape(T, H, W)
        Cb, Cr = g[..., ib], g[..., ir]
    return Y, Cb, Cr, ignored


def sample_mask(T, H, W, pix_fmt, pitches=None, offsets=None, frame_stride=None):
    """bool [T, frame_stride]: True where a byte belongs to a sample"""
    f = FORMATS[pix_fmt]
    ch, cw = chroma_shape(H, W, f.sub)
    zero = np.zeros((T, H, W), np.int64)
    zc = np.zeros((T, ch, cw), np.int64)
    return pack(zero, zc, zc, pix_fmt, pitches, offsets, frame_stride, fill=1) == 0


# ---- filters ---------------------------------------------------------------------------------------------------------------------------------
def upsample(c, sub, chroma, dtype):
    """chroma codes -> [T,H,W].  4:2:2: sample i is co-sited with luma column 2i; 'linear': even columns c[i], odd columns
    (c[i] + c[i+1]) / 2, clamped at the right edge; 'nearest': both columns c[i]."""
    if sub == 420:
        return M._upsample(c, chroma, dtype)
    c = c.astype(dtype)
    if sub == 444:
        return c
    if chroma == "nearest":
        return np.repeat(c, 2, axis=2)
    assert chroma == "linear"
    right = np.concatenate([c[:, :, 1:], c[:, :, -1:]], axis=2)
    out = np.empty(c.shape[:2] + (2 * c.shape[2],), dtype)
    out[:, :, 0::2] = c
    out[:, :, 1::2] = (c + right) / dtype(2)
    return out


def downsample(c, sub, chroma, dtype):
    """[T,H,W] -> the chroma plane.  4:2:2 'linear': [1 2 1] / 4 over columns 2i-1, 2i, 2i+1, edge-clamped; 'nearest': the mean of the two
    columns."""
    if sub == 420:
        return M._downsample(c, chroma, dtype)
    if sub == 444:
        return c
    if chroma == "nearest":
        return (c[:, :, 0::2] + c[:, :, 1::2]) / dtype(2)
    assert chroma == "linear"
    left = np.concatenate([c[:, :, :1], c[:, :, :-1]], axis=2)
    right = np.concatenate([c[:, :, 1:], c[:, :, -1:]], axis=2)
    return ((left + dtype(2) * c + right) / dtype(4))[:, :, 0::2]


def decode(Y, Cb, Cr, pix_fmt, matrix="bt709", full_range=False, chroma="linear", dtype=np.float64):
    """integer codes -> RGB [T,3,H,W], not clamped"""
    f = FORMATS[pix_fmt]
    dtype = np.dtype(dtype).type
    kr, kb = (dtype(v) for v in M.K[matrix])
    kg = dtype(1) - kr - kb
    y_off, y_sc, c_off, c_sc, _, _ = M._scales(f.bits, full_range, dtype)
    y = (Y.astype(dtype) - y_off) / y_sc
    cb = (upsample(Cb, f.sub, chroma, dtype) - c_off) / c_sc
    cr = (upsample(Cr, f.sub, chroma, dtype) - c_off) / c_sc
    r = y + dtype(2) * (dtype(1) - kr) * cr
    b = y + dtype(2) * (dtype(1) - kb) * cb
    g = y - (dtype(2) * kr * (dtype(1) - kr) / kg) * cr - (dtype(2) * kb * (dtype(1) - kb) / kg) * cb
    return np.stack([r, g, b], axis=1)


def encode_values(rgb, pix_fmt, matrix="bt709", full_range=False, chroma="linear", dtype=np.float64):
    """RGB [T,3,H,W] -> the scaled, clamped, NOT yet rounded code values (Y, Cb, Cr)"""
    f = FORMATS[pix_fmt]
    dtype = np.dtype(dtype).type
    kr, kb = (dtype(v) for v in M.K[matrix])
    kg = dtype(1) - kr - kb
    y_off, y_sc, c_off, c_sc, y_rng, c_rng = M._scales(f.bits, full_range, dtype)
    x = np.clip(rgb.astype(dtype), dtype(0), dtype(1))
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    yl = kr * r + kg * g + kb * b
    cb = downsample((b - yl) / (dtype(2) * (dtype(1) - kb)), f.sub, chroma, dtype)
    cr = downsample((r - yl) / (dtype(2) * (dtype(1) - kr)), f.sub, chroma, dtype)
    return (np.clip(yl * y_sc + y_off, *y_rng), np.clip(cb * c_sc + c_off, *c_rng), np.clip(cr * c_sc + c_off, *c_rng))


def encode(rgb, pix_fmt, **kw):
    """RGB -> integer codes (round half to even)"""
    return tuple(np.rint(v).astype(np.int64) for v in encode_values(rgb, pix_fmt, **kw))


def reflect_pad(x, Hp, Wp):
    """[..., H, W] -> [..., Hp, Wp]: element (r, c) = x[refl_H(r), refl_W(c)], refl_N(i) = i below N, else 2 (N - 1) - i"""
    H, W = x.shape[-2:]
    rows = [r if r < H else 2 * (H - 1) - r for r in range(Hp)]
    cols = [c if c < W else 2 * (W - 1) - c for c in range(Wp)]
    return x[..., rows, :][..., cols]
