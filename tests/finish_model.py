"""The output finish in numpy, written from the text of include/bsvd_hip.h (bsvd_blend_planar, BsvdDither) and independent of the library:
the blend, the 8 x 8 Bayer matrix with its per-component shifts, the hash and the dither value d, every operation in np.float32 in the
header's order -- and both dithers on top of the existing encoders' models (rgb_surface_model, yuv_surface_model, yuv_model: imported, not
edited).  The test model of tests/test_finish_cpu.py and tests/test_gpu_finish.py.

RGB: rgb_surface_model.encode in float32 IS the device's arithmetic, so ``rgb_to_surface`` is the device's bytes.  YUV: the existing models
state the encoder in another operation order (float64 for the truth), so ``yuv_codes`` returns the codes together with a mask of the samples
whose t + d lies within ``TIE`` of a rounding tie -- where fp32 noise of the encoder decides, as in the encoders' own GPU tests."""
import numpy as np

import rgb_surface_model as R
import yuv_model as M
import yuv_surface_model as S

f32 = np.float32
NONE, ORDERED, RANDOM = 0, 1, 2
MODES = {None: NONE, "ordered": ORDERED, "random": RANDOM}
SHIFTS = ((0, 0), (2, 5), (5, 2))                      # (r_c, q_c) of components 0, 1, 2
RANDOM_MAX = f32(0.5) - f32(2.0 ** -7)
TIE = 1e-3
LUMA_W = {name: (kr, 1.0 - kr - kb, kb) for name, (kr, kb) in M.K.items()}        # Kr, Kg, Kb as the encoders make them


def bayer(n=8):
    """the n x n Bayer matrix by the textbook recursion: B_2n = [[4 B, 4 B + 2], [4 B + 3, 4 B + 1]]"""
    b = np.zeros((1, 1), np.int64)
    while b.shape[0] < n:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


BAYER8 = bayer(8)


# ---- the blend -------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 arrays: a b is exact in float64, the sum with c rounds once to 53 bits and then to 24.  The two roundings can differ
    from fmaf's one only where the 53-bit sum is exactly a float32 tie; those elements (a few in 10^7 on random data) are redone in exact
    rationals, and where the exact sum IS the tie, fmaf's half-to-even result stands"""
    import fractions
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(f32)
    hazard = np.isfinite(s) & ((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28))
    for i in zip(*np.nonzero(hazard)):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        lo, hi = sorted((float(np.nextafter(out[i], f32(-np.inf))), float(np.nextafter(out[i], f32(np.inf)))))
        here = float(out[i])                                           # an EXACT tie keeps it: the float64 sum was exact and rounded half to even
        out[i] = min((here, lo, hi), key=lambda v: abs(fractions.Fraction(v) - exact))
    return out


def blend(y, x, s_luma, s_chroma, luma_w=LUMA_W["bt709"]):
    """y [T,3,H,W], x [T,>=3,H,W] float32 -> out [T,3,H,W]: m_c = s_c y_c + om x_c; l = fma(wB, dB, fma(wG, dG, wR dR)); out = m_c + dl l"""
    y, x = np.asarray(y, f32), np.asarray(x, f32)[:, :3]
    s_l, s_c = f32(s_luma), f32(s_chroma)
    om = f32(1.0 - float(s_c))
    dl = f32(s_c - s_l)
    w = [f32(v) for v in luma_w]
    d = x - y                                                     # float32, one subtraction per component
    l = fma32(w[2], d[:, 2], fma32(w[1], d[:, 1], w[0] * d[:, 0]))
    t = dl * l
    m = s_c * y + om * x
    return (m + t[:, None]).astype(f32)


def lerp(y, x, s):
    """the plain two-product lerp s y + (1 - s) x in float32"""
    s = f32(s)
    return (s * np.asarray(y, f32) + f32(1.0 - float(s)) * np.asarray(x, f32)[:, :3]).astype(f32)


# ---- the dither value ------------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    """MurmurHash3's 32-bit finaliser, on uint64 arrays holding 32-bit values"""
    h = np.asarray(h, np.uint64) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h


def d_ordered_entry(b):
    """d of matrix entry b (0 .. 63)"""
    return (np.asarray(b).astype(f32) + f32(0.5)) * f32(1.0 / 64) - f32(0.5)


def d_of_hash(h):
    """d of a 32-bit hash value: ((float)((int)(h >> 8) - 2^23) + 0.5f) * 2^-24, limited to +-(0.5 - 2^-7)"""
    k = (np.asarray(h, np.uint64) >> np.uint64(8)).astype(np.int64) - (1 << 23)
    d = (k.astype(f32) + f32(0.5)) * f32(2.0 ** -24)
    return np.clip(d, -RANDOM_MAX, RANDOM_MAX).astype(f32)


def frame_key(seed, frame, comp):
    n = (int(frame) * 4 + comp) & 0xffffffffffffffff
    return int(fmix32(seed ^ int(fmix32((n & 0xffffffff) ^ int(fmix32(n >> 32))))))


def hash32(seed, frame, comp, rows, cols):
    """h of the samples (rows x cols grids of equal shape) of one component of one frame (its STREAM index)"""
    p = (np.asarray(cols, np.uint64) + np.asarray(rows, np.uint64) * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)
    return fmix32(np.uint64(frame_key(seed, frame, comp)) ^ p)


def d_plane(mode, comp, h, w, seed=0, frame=0):
    """d [h, w] float32 of one component's own grid for the frame with stream index ``frame``; zeros with mode NONE"""
    mode = MODES.get(mode, mode)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if mode == NONE:
        return np.zeros((h, w), f32)
    if mode == ORDERED:
        r_c, q_c = SHIFTS[comp]
        return d_ordered_entry(BAYER8[(rows + r_c) & 7, (cols + q_c) & 7])
    return d_of_hash(hash32(seed, frame, comp, rows, cols))


def d_planes(mode, comp, T, h, w, seed=0, frame0=0, local_index=False):
    """d [T, h, w].  local_index: the MUTANT that hashes the call-local frame index where the stream index belongs"""
    return np.stack([d_plane(mode, comp, h, w, seed, t if local_index else frame0 + t) for t in range(T)])


def quantise(t, d, lo, hi, rgb_order=False):
    """the encoders' rounding of scaled float32 values t with dither d: YUV rint(clamp(t + d)), RGB clamp(rint(t + d))"""
    v = (np.asarray(t, f32) + np.asarray(d, f32)).astype(f32)
    return (np.clip(np.rint(v), lo, hi) if rgb_order else np.rint(np.clip(v, f32(lo), f32(hi)))).astype(np.int64)


# ---- on top of the encoders' models ----------------------------------------------------------------------------------------------------------
def rgb_codes(v, bits, full_range, mode, comp, seed=0, frame0=0, local_index=False):
    """values [T,H,W] of component ``comp`` -> codes: rgb_surface_model.encode's arithmetic with d joining before rintf"""
    s = 1 << (bits - 8)
    mul, add, hi = (f32((1 << bits) - 1), f32(0), (1 << bits) - 1) if full_range else (f32(219 * s), f32(16 * s), 235 * s)
    x = np.clip(np.where(np.isnan(v), f32(0), v).astype(f32), f32(0), f32(1))
    t = x * mul + add
    T, H, W = t.shape
    return quantise(t, d_planes(mode, comp, T, H, W, seed, frame0, local_index), float(add), hi, rgb_order=True)


def rgb_to_surface(y, name, full_range=True, pitches=None, offsets=None, frame_stride=None, crop_to=None, alpha=None, fill=0, mode=None, seed=0,
                   frame0=0, local_index=False):
    """bsvd_planar_to_rgb_d: rgb_surface_model.to_surface with dithered R, G, B; the fourth sample is what it is there"""
    f = R.FORMATS[name]
    H, W = crop_to if crop_to is not None else y.shape[-2:]
    y = np.asarray(y, f32)[:, :, :H, :W]
    top = (1 << f.bits) - 1
    fourth = None
    if len(f.order) == 4:
        fourth = np.full((y.shape[0], H, W), top, np.int64) if alpha is None or R.has_filler(name) else alpha.astype(np.int64) & top
    codes = [rgb_codes(y[:, c], f.bits, full_range, mode, c, seed, frame0, local_index) for c in range(3)]
    if MODES.get(mode, mode) == NONE:
        assert all(np.array_equal(codes[c], R.encode(y[:, c], f.bits, full_range)) for c in range(3))
    return R.pack(codes[0], codes[1], codes[2], name, fourth, pitches, offsets, frame_stride, fill=fill, x_ones=True)


def _yuv_finish(vals, ranges, mode, seed, frame0, luma_grid_chroma, local_index):
    """(Y, Cb, Cr) scaled, clamped float64 values -> ([codes], [near-tie masks]); luma_grid_chroma: the MUTANT that indexes subsampled chroma
    by the luma grid (row * ry, col * rx) instead of its own"""
    codes, ties = [], []
    T, H, W = vals[0].shape
    for comp, (v, (lo, hi)) in enumerate(zip(vals, ranges)):
        _, h, w = v.shape
        if luma_grid_chroma and (h, w) != (H, W):
            d = np.stack([d_plane(mode, comp, H, W, seed, t if local_index else frame0 + t)[::H // h, ::W // w] for t in range(T)])
        else:
            d = d_planes(mode, comp, T, h, w, seed, frame0, local_index)
        t = v + d.astype(np.float64)
        codes.append(np.rint(np.clip(t, lo, hi)).astype(np.int64))
        ties.append(np.abs(t - np.floor(t) - 0.5) <= TIE)
    return codes, ties


def _ranges(bits, full_range):
    _, _, _, _, y_rng, c_rng = M._scales(bits, full_range, np.float64)
    return [tuple(float(v) for v in y_rng)] + [tuple(float(v) for v in c_rng)] * 2


def yuv_codes(rgb, pix_fmt, mode=None, seed=0, frame0=0, luma_grid_chroma=False, local_index=False, **kw):
    """bsvd_planar_to_yuv_crop_d on the picture rgb [T,3,H,W] -> ([Y, Cb, Cr] codes, [near-tie masks])"""
    vals = S.encode_values(rgb, pix_fmt, dtype=np.float64, **kw)
    return _yuv_finish(vals, _ranges(S.FORMATS[pix_fmt].bits, kw.get("full_range", False)), mode, seed, frame0, luma_grid_chroma, local_index)


def yuv420_codes(rgb, pix_fmt, mode=None, seed=0, frame0=0, luma_grid_chroma=False, local_index=False, **kw):
    """bsvd_planar_to_yuv420_crop_d (nv12 / p010) likewise"""
    bits = M.BITS[pix_fmt]
    vals = M.encode_values(rgb, bits, dtype=np.float64, **kw)
    return _yuv_finish(vals, _ranges(bits, kw.get("full_range", False)), mode, seed, frame0, luma_grid_chroma, local_index)


# ---- the inputs of the device comparison (tests/test_gpu_finish.py; the mutants of tests/test_finish_cpu.py must fail on them) ------------------
T = 3
FRAME0 = 5
SEED = 0x5eed1234
PICTURES = [((10, 22), (16, 24)), ((12, 18), (16, 24)), ((16, 32), (16, 32))]           # (picture, tensor): rows ending in part items of 2
RGB_NAMES_444 = ("yuv444p", "yuv444p10le")


def values(Hp, Wp, lo=-0.1, hi=1.1):
    """seeded float32 [T,3,Hp,Wp]: uniform(lo, hi), beyond both clamps, with 40 % of the 4 x 4 blocks one corner of the RGB cube (or beyond
    it: a 1 may be 1.5, a 0 may be -0.5) -- flat patches wide enough for the chroma filters, so that limited range meets the legal ends of
    luma (black, white) and of chroma (blue, yellow, red, cyan) on both sides"""
    rs = np.random.RandomState(7 * Hp + Wp)
    x = rs.uniform(lo, hi, (T, 3, Hp, Wp))
    hb, wb = (Hp + 3) // 4, (Wp + 3) // 4
    corner = rs.randint(0, 2, (T, 3, hb, wb)).astype(np.float64)
    corner = np.where(rs.uniform(size=corner.shape) < 0.5, corner, np.where(corner > 0.5, 1.5, -0.5))
    pick = rs.uniform(size=(T, 1, hb, wb)) < 0.4
    up = lambda a: np.repeat(np.repeat(a, 4, axis=2), 4, axis=3)[:, :, :Hp, :Wp]
    return np.where(up(pick), up(corner), x).astype(f32)


def mismatches(got, want, ties):
    """samples where codes ``got`` differ from the model's ``want``, a step of 1 at a near-tie of the model excepted (the rule of the YUV
    encoders' own tests: there fp32 noise of the encoder decides)"""
    n = 0
    for g, w, t in zip(got, want, ties):
        d = np.asarray(g, np.int64) - w
        n += int(((d != 0) & ~(t & (np.abs(d) == 1))).sum())
    return n
