"""YUV 4:2:0 <-> RGB in numpy, written from the formulas of include/bsvd_hip.h (bsvd_yuv420_to_planar / bsvd_planar_to_yuv420) and
independent of the library: the test model of tests/test_yuv_cpu.py and tests/test_gpu_yuv.py.  ``dtype`` is the arithmetic's type:
float64 for the truth, float32 for what fp32 arithmetic in this order gives.  Planes are arrays of integer codes [T,H,W] (Y) and
[T,H/2,W/2] (Cb, Cr); ``pack`` / ``unpack`` move them into and out of pitched NV12 / P010 byte buffers."""
import numpy as np

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}      # (Kr, Kb)
BITS = {"nv12": 8, "p010": 10}


def _scales(bits, full_range, dtype):
    """-> y offset, y scale, chroma offset, chroma scale, (y lo, y hi), (c lo, c hi) in codes"""
    s = 2 ** (bits - 8)
    top = 2 ** bits - 1
    if full_range:
        return dtype(0), dtype(top), dtype(2 ** (bits - 1)), dtype(top), (0, top), (0, top)
    return dtype(16 * s), dtype(219 * s), dtype(128 * s), dtype(224 * s), (16 * s, 235 * s), (16 * s, 240 * s)


def _upsample(c, chroma, dtype):
    """[T,H/2,W/2] codes -> [T,H,W]"""
    c = c.astype(dtype)
    if chroma == "nearest":
        return np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    assert chroma == "linear"
    T, hh, wh = c.shape
    up = np.concatenate([c[:, :1], c[:, :-1]], axis=1)            # c[j-1], clamped
    dn = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)            # c[j+1], clamped
    v = np.empty((T, 2 * hh, wh), dtype)
    v[:, 0::2] = up / dtype(4) + dtype(3) * c / dtype(4)
    v[:, 1::2] = dtype(3) * c / dtype(4) + dn / dtype(4)
    right = np.concatenate([v[:, :, 1:], v[:, :, -1:]], axis=2)   # c[i+1], clamped
    out = np.empty((T, 2 * hh, 2 * wh), dtype)
    out[:, :, 0::2] = v
    out[:, :, 1::2] = (v + right) / dtype(2)
    return out


def decode(Y, Cb, Cr, bits, matrix="bt709", full_range=False, chroma="linear", dtype=np.float64):
    """integer codes -> RGB [T,3,H,W], not clamped"""
    dtype = np.dtype(dtype).type
    kr, kb = (dtype(v) for v in K[matrix])
    kg = dtype(1) - kr - kb
    y_off, y_sc, c_off, c_sc, _, _ = _scales(bits, full_range, dtype)
    y = (Y.astype(dtype) - y_off) / y_sc
    cb = (_upsample(Cb, chroma, dtype) - c_off) / c_sc
    cr = (_upsample(Cr, chroma, dtype) - c_off) / c_sc
    r = y + dtype(2) * (dtype(1) - kr) * cr
    b = y + dtype(2) * (dtype(1) - kb) * cb
    g = y - (dtype(2) * kr * (dtype(1) - kr) / kg) * cr - (dtype(2) * kb * (dtype(1) - kb) / kg) * cb
    return np.stack([r, g, b], axis=1)


def _downsample(c, chroma, dtype):
    """[T,H,W] -> [T,H/2,W/2]"""
    if chroma == "nearest":
        return (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]) / dtype(4)
    assert chroma == "linear"
    m = (c[:, 0::2] + c[:, 1::2]) / dtype(2)
    left = np.concatenate([m[:, :, :1], m[:, :, :-1]], axis=2)    # column x - 1, clamped
    right = np.concatenate([m[:, :, 1:], m[:, :, -1:]], axis=2)   # column x + 1, clamped
    f = (left + dtype(2) * m + right) / dtype(4)
    return f[:, :, 0::2]


def encode_values(rgb, bits, matrix="bt709", full_range=False, chroma="linear", dtype=np.float64):
    """RGB [T,3,H,W] -> the scaled, clamped, NOT yet rounded code values (Y [T,H,W], Cb, Cr [T,H/2,W/2])"""
    dtype = np.dtype(dtype).type
    kr, kb = (dtype(v) for v in K[matrix])
    kg = dtype(1) - kr - kb
    y_off, y_sc, c_off, c_sc, y_rng, c_rng = _scales(bits, full_range, dtype)
    x = np.clip(rgb.astype(dtype), dtype(0), dtype(1))
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    yl = kr * r + kg * g + kb * b
    cb = _downsample((b - yl) / (dtype(2) * (dtype(1) - kb)), chroma, dtype)
    cr = _downsample((r - yl) / (dtype(2) * (dtype(1) - kr)), chroma, dtype)
    return (np.clip(yl * y_sc + y_off, *y_rng), np.clip(cb * c_sc + c_off, *c_rng), np.clip(cr * c_sc + c_off, *c_rng))


def encode(rgb, bits, **kw):
    """RGB -> integer codes (round half to even)"""
    return tuple(np.rint(v).astype(np.int64) for v in encode_values(rgb, bits, **kw))


# ---- pitched byte buffers ----------------------------------------------------------------------------------------------------------
def frame_bytes(H, W, pix_fmt, row_pitch=None):
    return (row_pitch or W * (2 if pix_fmt == "p010" else 1)) * H * 3 // 2


def pack(Y, Cb, Cr, pix_fmt, row_pitch=None, frame_stride=None, fill=0, low_bits=None):
    """codes -> uint8 [T, frame_stride]: Y plane, then interleaved CbCr, rows ``row_pitch`` bytes apart; every byte that is not a
    sample is ``fill``.  P010: word = code << 6 (| low_bits, an array of junk for the 6 bits a reader must ignore)."""
    T, H, W = Y.shape
    sb = 2 if pix_fmt == "p010" else 1
    pitch = row_pitch or W * sb
    stride = frame_stride or pitch * H * 3 // 2
    rows = np.concatenate([Y, np.stack([Cb, Cr], axis=-1).reshape(T, H // 2, W)], axis=1)        # [T, H*3/2, W] samples
    if sb == 2:
        words = (rows.astype(np.uint16) << 6) | (0 if low_bits is None else (low_bits.astype(np.uint16) & 63))
        raw = words.astype("<u2").view(np.uint8).reshape(T, H * 3 // 2, W * 2)
    else:
        raw = rows.astype(np.uint8)
    buf = np.full((T, stride), fill, np.uint8)
    surf = buf[:, :pitch * H * 3 // 2].reshape(T, H * 3 // 2, pitch)
    surf[:, :, :W * sb] = raw
    return buf


def unpack(buf, H, W, pix_fmt, row_pitch=None):
    """uint8 [T, >= frame_bytes] -> (Y, Cb, Cr, words): integer codes and, for P010, the raw 16-bit words [T, H*3/2, W] (else None)"""
    T = buf.shape[0]
    sb = 2 if pix_fmt == "p010" else 1
    pitch = row_pitch or W * sb
    raw = np.ascontiguousarray(buf[:, :pitch * H * 3 // 2].reshape(T, H * 3 // 2, pitch)[:, :, :W * sb])
    words = None
    if sb == 2:
        words = raw.view("<u2").astype(np.int64)
        rows = words >> 6
    else:
        rows = raw.astype(np.int64)
    c = rows[:, H:].reshape(T, H // 2, W // 2, 2)
    return rows[:, :H], c[..., 0], c[..., 1], words


def sample_mask(T, H, W, pix_fmt, row_pitch=None, frame_stride=None):
    """bool [T, frame_stride]: True where a byte belongs to a sample (False: pitch padding and the bytes between frames)"""
    one = np.ones((T, H, W), np.int64)
    half = np.ones((T, H // 2, W // 2), np.int64)
    m = pack(one * 0, half * 0, half * 0, pix_fmt, row_pitch, frame_stride, fill=1)
    return m == 0
