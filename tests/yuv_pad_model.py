"""The pad / crop rule of the frame I/O entry points (include/bsvd_hip.h, bsvd_*_pad / bsvd_*_crop) in numpy, on top of tests/yuv_model.py:
in = the model's decode at picture size, then ``np.pad(mode='reflect')`` on the right and bottom; out = slice to the picture, then the model's
encode.  Shared by tests/test_frame_pad_cpu.py and tests/test_gpu_frame_pad.py, with the seeded inputs both use."""
import functools

import numpy as np

import yuv_model as M


def pad_reflect(x, Hp, Wp):
    """[..., H, W] -> [..., Hp, Wp]: right / bottom reflect pad, the edge sample not repeated (torch's 'reflect', golden g8's rule)"""
    H, W = x.shape[-2:]
    return np.pad(x, [(0, 0)] * (x.ndim - 2) + [(0, Hp - H), (0, Wp - W)], mode="reflect")


def decode_pad(Y, Cb, Cr, bits, Hp, Wp, **kw):
    """integer codes of an H x W picture -> RGB [T,3,Hp,Wp]"""
    return pad_reflect(M.decode(Y, Cb, Cr, bits, **kw), Hp, Wp)


def encode_values_crop(rgb, H, W, bits, **kw):
    """RGB [T,3,Hp,Wp] -> the unrounded code values of its H x W picture"""
    return M.encode_values(rgb[..., :H, :W], bits, **kw)


# (H, W) -> (Hp, Wp) with W % 4 == 2 (a half item at the right edge) and / or an odd number of row pairs
HALF_ITEM_SIZES = [((6, 6), (8, 8)), ((6, 10), (8, 12)), ((30, 42), (32, 44)), ((34, 52), (36, 52))]
T = 2


@functools.lru_cache(maxsize=None)
def codes(pix_fmt, T, H, W):
    """seeded random codes over the full code range (+ junk for the low 6 bits of P010 words); shared, never written"""
    rs = np.random.RandomState(1000 * T + 10 * H + W)
    top = 2 ** M.BITS[pix_fmt]
    out = (rs.randint(0, top, (T, H, W)), rs.randint(0, top, (T, H // 2, W // 2)), rs.randint(0, top, (T, H // 2, W // 2)),
           rs.randint(0, 64, (T, H * 3 // 2, W)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rgb(T, H, W, lo=-0.1, hi=1.1):
    """seeded RGB with values outside [0,1]; shared, never written"""
    x = np.random.RandomState(7 * T + 3 * H + W).uniform(lo, hi, (T, 3, H, W)).astype(np.float32)
    x.setflags(write=False)
    return x


def near_half(vals, eps=1e-3):
    """per plane: where the unrounded value lies within eps of a half-integer (there a conforming fp32 encoder may round the other way)"""
    return [np.abs(v - np.floor(v) - 0.5) <= eps for v in vals]
