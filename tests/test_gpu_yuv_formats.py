"""The planar, 4:2:2 and 4:4:4 YUV surfaces on the device (bsvd_amd/csrc/frame_yuv.hip through frame_io.yuv_to_input /
output_to_yuv and the pipelines' pix_fmt): bit for bit against the NV12 / P010 kernels where the formats say the same thing, against the
independent numpy model tests/yuv_surface_model.py elsewhere, and the memory contract.  T = 2.  Pictures: 4x4 is one item with both edge
clamps in one chroma sample, 8x12 an odd item count per row, 12x20 and 36x52 several rows of items with every neighbour case; the pad /
crop pictures 6x10 (4:2:0), 5x10 (4:2:2), 5x7 (4:4:4) end their rows in part items and pad both ways.  Every layout also runs pitched, with
plane offsets, gaps between planes and frames, and 0xFF (a NaN pattern to any float reader) in every byte that is no sample."""
import functools
import itertools

import numpy as np
import pytest
import torch

import yuv_model as M
import yuv_surface_model as S
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

T = 2
SIZES = [(4, 4), (8, 12), (12, 20), (36, 52)]
PAD_PICTURE = {420: (6, 10), 422: (5, 10), 444: (5, 7)}
PAD_420 = [((6, 10), (8, 12)), ((10, 14), (16, 24))]      # picture, tensor: 4:2:0 against NV12 / P010 through pad and crop
NAMES = sorted(S.FORMATS)
COLOUR = list(itertools.product(["bt601", "bt709", "bt2020"], [False, True], ["nearest", "linear"]))
GUARD = 66          # bytes in front of a surface inside its allocation: surfaces promise no more than their sample's alignment
SIGMA = 30 / 255.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _layouts(H, W, pix_fmt):
    """(pitches, offsets, frame_stride): tight; and rows rounded up to 64 bytes plus 64 and a bit, plane 0 66 bytes into the frame, gaps of
    34 and 18 bytes behind planes 0 and 1, frames one frame plus 128 bytes apart"""
    pl = S.planes(H, W, pix_fmt)
    pitches = [(rb + 63) // 64 * 64 + 64 + 2 * i for i, (_, rb) in enumerate(pl)]
    offsets, at = [], 66
    for i, (rows, _) in enumerate(pl):
        offsets.append(at)
        at += pitches[i] * rows + (34, 18, 0)[i]
    return [(None, None, None), (pitches, offsets, S.frame_bytes(H, W, pix_fmt, pitches, offsets) + 128)]


@functools.lru_cache(maxsize=None)
def _codes(bits, sub, H, W):
    """seeded random codes over the full code range; shared, never written"""
    rs = np.random.RandomState(100 * H + W + bits + sub)
    top = 2 ** bits
    ch, cw = S.chroma_shape(H, W, sub)
    out = (rs.randint(0, top, (T, H, W)), rs.randint(0, top, (T, ch, cw)), rs.randint(0, top, (T, ch, cw)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _rgb(H, W, kind):
    """'uniform': seeded uniform(-0.1, 1.1).  'limits': 70 % of the pixels are white, black, red, green, blue or magenta, at the gamut's
    corner or beyond it (a 1 may be 1.5, a 0 may be -0.5), the rest uniform: luma at both ends of the legal range, chroma at its upper end,
    flat runs and the hardest edges for the chroma filters.  Yellow and cyan are left out: their Cb / Cr of exactly -1/2 is, in full range,
    the code 0.5 -- a rounding tie by construction, which the tie rule would only exclude.  Shared, never written."""
    rs = np.random.RandomState(3 * H + W + len(kind))
    x = rs.uniform(-0.1, 1.1, (T, 3, H, W))
    if kind == "limits":
        palette = np.array([(1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)], np.float64)
        corner = np.moveaxis(palette[rs.randint(0, len(palette), (T, H, W))], -1, 1)
        corner = np.where(rs.uniform(size=x.shape) < 0.5, corner, np.where(corner > 0.5, 1.5, -0.5))
        x = np.where(rs.uniform(size=(T, 1, H, W)) < 0.7, corner, x)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _surface(buf, fill):
    """host surface [T, stride] -> device view of the same bytes inside a larger allocation filled with ``fill``"""
    n, stride = buf.shape
    big = torch.full((GUARD + n * stride + GUARD,), fill, dtype=torch.uint8, device="cuda:0")
    view = big[GUARD:GUARD + n * stride].view(n, stride)
    view.copy_(torch.from_numpy(buf))
    return big, view


def _decode(buf, H, W, fill=0xFF, **kw):
    from bsvd_amd.frame_io import yuv_to_input
    _, view = _surface(buf, fill)
    return yuv_to_input(view, H, W, **kw).cpu().numpy()


def _decode420(buf, H, W, **kw):
    from bsvd_amd.frame_io import yuv420_to_input
    _, view = _surface(buf, 0xFF)
    return yuv420_to_input(view, H, W, **kw).cpu().numpy()


def _encode(x, stride, **kw):
    """-> (the surface [T, stride], the whole allocation around it) after an encode into memory prefilled with 0xA5"""
    from bsvd_amd.frame_io import output_to_yuv
    big, view = _surface(np.full((x.shape[0], stride), 0xA5, np.uint8), 0xA5)
    got = output_to_yuv(torch.tensor(x, device="cuda:0"), out=view, **kw)
    assert got.data_ptr() == view.data_ptr()
    return view.cpu().numpy(), big.cpu().numpy()


def _encode420(x, pix_fmt, **kw):
    from bsvd_amd.frame_io import output_to_yuv420
    return output_to_yuv420(torch.tensor(x, device="cuda:0"), pix_fmt=pix_fmt, **kw).cpu().numpy()


# ---- against the existing kernels, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt,semi", [("yuv420p", "nv12"), ("yuv420p10le", "p010")])
def test_planar_420_is_the_semi_planar_kernel_bit_for_bit(pix_fmt, semi):
    """yuv420p decodes to exactly the tensor bsvd_yuv420_to_planar gives for the same samples as NV12, and encodes to exactly its codes, for
    every matrix x range x chroma; likewise yuv420p10le and P010.  The ignored bits of the two 10-bit rules hold different junk.  The same
    through the pad and crop entry points, at pictures that end their rows in a half item and pad both ways, by less and by more than one
    item: one kernel serves both formats, so this holds its semi-planar loads and stores against its planar ones."""
    bits = S.FORMATS[pix_fmt].bits
    rs = np.random.RandomState(5)
    for (H, W), (matrix, full_range, chroma) in itertools.product(SIZES, COLOUR):
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        Y, Cb, Cr = _codes(bits, 420, H, W)
        want = _decode420(M.pack(Y, Cb, Cr, semi, low_bits=rs.randint(0, 64, (T, H * 3 // 2, W))), H, W, pix_fmt=semi, sigma=SIGMA, **kw)
        got = _decode(S.pack(Y, Cb, Cr, pix_fmt, junk=rs), H, W, pix_fmt=pix_fmt, sigma=SIGMA, **kw)
        assert np.array_equal(_bits(got), _bits(want)), (H, W, kw)
        for kind in ("uniform", "limits"):
            x = _rgb(H, W, kind)
            y1, cb1, cr1, _ = M.unpack(_encode420(x, semi, **kw), H, W, semi)
            surf, _ = _encode(x, S.frame_bytes(H, W, pix_fmt), pix_fmt=pix_fmt, **kw)
            y2, cb2, cr2, ignored = S.unpack(surf, H, W, pix_fmt)
            assert np.array_equal(y1, y2) and np.array_equal(cb1, cb2) and np.array_equal(cr1, cr2) and ignored == 0, (H, W, kw, kind)
    for ((H, W), pad), (matrix, full_range, chroma) in itertools.product(PAD_420, COLOUR):
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        Y, Cb, Cr = _codes(bits, 420, H, W)
        want = _decode420(M.pack(Y, Cb, Cr, semi, low_bits=rs.randint(0, 64, (T, H * 3 // 2, W))), H, W, pix_fmt=semi, sigma=SIGMA, pad_to=pad, **kw)
        got = _decode(S.pack(Y, Cb, Cr, pix_fmt, junk=rs), H, W, pix_fmt=pix_fmt, sigma=SIGMA, pad_to=pad, **kw)
        assert got.shape == (T, 4) + pad and np.array_equal(_bits(got), _bits(want)), (H, W, pad, kw)
        for kind in ("uniform", "limits"):
            x = _rgb(pad[0], pad[1], kind)
            y1, cb1, cr1, _ = M.unpack(_encode420(x, semi, crop_to=(H, W), **kw), H, W, semi)
            surf, _ = _encode(x, S.frame_bytes(H, W, pix_fmt), pix_fmt=pix_fmt, crop_to=(H, W), **kw)
            y2, cb2, cr2, ignored = S.unpack(surf, H, W, pix_fmt)
            assert np.array_equal(y1, y2) and np.array_equal(cb1, cb2) and np.array_equal(cr1, cr2) and ignored == 0, (H, W, pad, kw, kind)


@pytest.mark.parametrize("bits", [8, 10])
def test_nearest_422_and_444_of_replicated_chroma_equal_420(bits):
    """chroma='nearest': a 4:2:2 surface whose chroma rows are duplicated in pairs, and a 4:4:4 surface holding the nearest-upsampled
    chroma, decode bit-equal to the 4:2:0 surface (the NV12 / P010 kernel)."""
    semi = "nv12" if bits == 8 else "p010"
    f422 = ["nv16", "yuv422p", "uyvy422", "yuyv422"] if bits == 8 else ["p210le", "yuv422p10le"]
    f444 = "yuv444p" if bits == 8 else "yuv444p10le"
    for (H, W), matrix, full_range in itertools.product(SIZES, ["bt601", "bt709", "bt2020"], [False, True]):
        kw = dict(matrix=matrix, full_range=full_range, chroma="nearest")
        Y, Cb, Cr = _codes(bits, 420, H, W)
        want = _decode420(M.pack(Y, Cb, Cr, semi), H, W, pix_fmt=semi, **kw)
        cb2, cr2 = np.repeat(Cb, 2, axis=1), np.repeat(Cr, 2, axis=1)
        for name in f422:
            got = _decode(S.pack(Y, cb2, cr2, name), H, W, pix_fmt=name, **kw)
            assert np.array_equal(_bits(got), _bits(want)), (name, H, W, kw)
        got = _decode(S.pack(Y, np.repeat(cb2, 2, axis=2), np.repeat(cr2, 2, axis=2), f444), H, W, pix_fmt=f444, **kw)
        assert np.array_equal(_bits(got), _bits(want)), (f444, H, W, kw)


@pytest.mark.parametrize("names", [("uyvy422", "yuyv422", "nv16", "yuv422p"), ("p210le", "yuv422p10le")])
def test_422_layouts_agree_bit_for_bit(names):
    """the same samples in every 4:2:2 layout of one bit depth: the same tensor in, and from the same tensor the same codes out"""
    bits = S.FORMATS[names[0]].bits
    rs = np.random.RandomState(6)
    for (H, W), (matrix, full_range, chroma) in itertools.product(SIZES, COLOUR):
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        Y, Cb, Cr = _codes(bits, 422, H, W)
        x = _rgb(H, W, "limits")
        first = None
        for name in names:
            got = _decode(S.pack(Y, Cb, Cr, name, junk=rs), H, W, pix_fmt=name, **kw)
            surf, _ = _encode(x, S.frame_bytes(H, W, name), pix_fmt=name, **kw)
            codes = S.unpack(surf, H, W, name)[:3]
            if first is None:
                first = (got, codes)
            assert np.array_equal(_bits(got), _bits(first[0])), (name, H, W, kw)
            assert all(np.array_equal(a, b) for a, b in zip(codes, first[1])), (name, H, W, kw)


# ---- against the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", NAMES)
def test_decode_matches_the_float64_model(pix_fmt):
    """max-abs <= 1e-6 on values of O(1), the bound of the NV12 / P010 decode.  Random codes over the full code range; the sigma channel is
    bit-equal to float32(sigma); a pitched surface with plane offsets whose padding, gaps and surroundings hold 0xFF bytes and whose
    ignored bits hold junk decodes to the bits of the tight, clean one."""
    f = S.FORMATS[pix_fmt]
    rs = np.random.RandomState(7)
    worst = 0.0
    for (H, W), (matrix, full_range, chroma) in itertools.product(SIZES, COLOUR):
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        Y, Cb, Cr = _codes(f.bits, f.sub, H, W)
        want = S.decode(Y, Cb, Cr, pix_fmt, dtype=np.float64, **kw)
        results = []
        for (pitches, offsets, stride), junk in zip(_layouts(H, W, pix_fmt), (None, rs)):
            buf = S.pack(Y, Cb, Cr, pix_fmt, pitches, offsets, stride, fill=0xFF, junk=junk)
            got = _decode(buf, H, W, pix_fmt=pix_fmt, sigma=SIGMA, pitches=pitches, offsets=offsets, **kw)
            assert got.shape == (T, 4, H, W) and got.dtype == np.float32
            assert (_bits(got[:, 3]) == np.float32(SIGMA).view(np.uint32)).all()
            err = float(np.abs(got[:, :3].astype(np.float64) - want).max())
            worst = max(worst, err)
            assert err <= 1e-6, (H, W, kw, pitches, err)
            results.append(got)
        assert np.array_equal(_bits(results[0]), _bits(results[1])), (H, W, kw)
    blind = _decode(S.pack(Y, Cb, Cr, pix_fmt), H, W, pix_fmt=pix_fmt, **kw)                          # no sigma: three channels
    assert blind.shape == (T, 3, H, W) and np.array_equal(_bits(blind), _bits(results[0][:, :3]))
    print("decode %s: max-abs vs float64 model %.3e" % (pix_fmt, worst))


def _check_codes(planes, vals, band, where):
    for name, got, v, b in zip("Y Cb Cr".split(), planes, vals, band):
        d = got - np.rint(v).astype(np.int64)
        bad = (d != 0) & ~(b & (np.abs(d) == 1))
        assert not bad.any(), where + (name, int(bad.sum()), got[bad][:4], v[bad][:4])


@pytest.mark.parametrize("kind", ["uniform", "limits"])
@pytest.mark.parametrize("pix_fmt", NAMES)
def test_encode_matches_the_float64_model(pix_fmt, kind):
    """Codes equal rint of the float64 model except where its pre-rounding value lies within 1e-3 of a half-integer (there +-1 is accepted);
    such samples are at most 1 % of the samples of a case -- one format, input set, matrix, range and chroma filter over the four pictures,
    as in the NV12 / P010 test --, asserted on the model before the kernel runs (uniform values put 2 x 1e-3 = 0.2 % there).  The ignored
    bits of 10-bit words are zero.  Guard bytes around the surface, pitch padding, the gaps between planes and between frames keep their
    0xA5."""
    for matrix, full_range, chroma in COLOUR:
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        model = []
        for H, W in SIZES:
            vals = S.encode_values(_rgb(H, W, kind), pix_fmt, dtype=np.float64, **kw)
            model.append((vals, [np.abs(v - np.floor(v) - 0.5) <= 1e-3 for v in vals]))
        near, total = sum(int(b.sum()) for _, band in model for b in band), sum(b.size for _, band in model for b in band)
        assert near <= 0.01 * total, (kw, near, total)
        for (H, W), (vals, band) in zip(SIZES, model):
            x = _rgb(H, W, kind)
            for pitches, offsets, stride in _layouts(H, W, pix_fmt):
                stride = stride or S.frame_bytes(H, W, pix_fmt)
                surf, big = _encode(x, stride, pix_fmt=pix_fmt, pitches=pitches, offsets=offsets, **kw)
                planes = S.unpack(surf, H, W, pix_fmt, pitches, offsets)
                _check_codes(planes, vals, band, (H, W, kw, pitches))
                assert planes[3] == 0
                mask = S.sample_mask(T, H, W, pix_fmt, pitches, offsets, stride)
                assert (surf[~mask] == 0xA5).all(), (H, W, kw, pitches)
                assert (big[:GUARD] == 0xA5).all() and (big[-GUARD:] == 0xA5).all(), (H, W, kw, pitches)


def test_output_without_out_allocates_a_zero_padded_surface():
    from bsvd_amd.frame_io import output_to_yuv, yuv_frame_bytes
    H, W = 12, 20
    x = torch.tensor(_rgb(H, W, "uniform"), device="cuda:0")
    for pix_fmt in ("yuv420p", "uyvy422", "p210le", "yuv444p10le"):
        for pitches, offsets, _ in _layouts(H, W, pix_fmt):
            got = output_to_yuv(x, pix_fmt, pitches=pitches, offsets=offsets)
            assert got.shape == (T, yuv_frame_bytes(H, W, pix_fmt, pitches, offsets)) and got.dtype == torch.uint8
            surf, _ = _encode(x.cpu().numpy(), got.shape[1], pix_fmt=pix_fmt, pitches=pitches, offsets=offsets)
            mask = S.sample_mask(T, H, W, pix_fmt, pitches, offsets)
            got = got.cpu().numpy()
            assert np.array_equal(got[mask], surf[mask])
            if pitches:
                assert (got[~mask] == 0).all()


# ---- pad and crop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", NAMES)
def test_pad_mirrors_the_converted_picture(pix_fmt):
    """pad_to: every pad element is bit-equal to its mirror source, the picture region is within 1e-6 of the model's conversion at picture
    size (chroma clamped at the PICTURE's edges), the constant channel is constant over the whole plane; and where the unpadded conversion
    can run (a picture whose W is a multiple of 4, converted with pad_to = its own size) the result is bit-equal to
    denoise.pad_to_multiple_of_4 of it.  Tight and pitched."""
    from bsvd_amd.denoise import pad_to_multiple_of_4
    from bsvd_amd.frame_io import network_size
    f = S.FORMATS[pix_fmt]
    H0, W0 = PAD_PICTURE[f.sub]
    for (H, W), (matrix, full_range, chroma) in itertools.product([(H0, W0), (H0, W0 + (4 - W0 % 4) % 4 if W0 % 4 else W0)], COLOUR):
        kw = dict(pix_fmt=pix_fmt, matrix=matrix, full_range=full_range, chroma=chroma)
        Hp, Wp = network_size(H, W)
        Y, Cb, Cr = _codes(f.bits, f.sub, H, W)
        want = S.decode(Y, Cb, Cr, dtype=np.float64, **kw)
        for pitches, offsets, stride in _layouts(H, W, pix_fmt):
            buf = S.pack(Y, Cb, Cr, pix_fmt, pitches, offsets, stride, fill=0xFF)
            got = _decode(buf, H, W, sigma=SIGMA, pitches=pitches, offsets=offsets, pad_to=(Hp, Wp), **kw)
            assert got.shape == (T, 4, Hp, Wp)
            assert np.array_equal(_bits(got), _bits(S.reflect_pad(got[..., :H, :W], Hp, Wp))), (H, W, kw, pitches)
            assert (_bits(got[:, 3]) == np.float32(SIGMA).view(np.uint32)).all()
            assert np.abs(got[:, :3, :H, :W].astype(np.float64) - want).max() <= 1e-6, (H, W, kw, pitches)
            if W % 4 == 0:
                _, view = _surface(buf, 0xFF)
                from bsvd_amd.frame_io import yuv_to_input
                plain = yuv_to_input(view, H, W, sigma=SIGMA, pitches=pitches, offsets=offsets, pad_to=(H, W), **kw)
                assert plain.shape == (T, 4, H, W)
                padded = pad_to_multiple_of_4(plain)[0].cpu().numpy()
                assert np.array_equal(_bits(got), _bits(padded)), (H, W, kw, pitches)


@pytest.mark.parametrize("pix_fmt", NAMES)
def test_crop_reads_the_picture_only(pix_fmt):
    """crop_to: the codes of the model's conversion of y[..., :H, :W] (the tie rule of the encode test, its 1 % cap over the format's twelve
    colour settings together, asserted on the model first), the same bytes whether the pad region of y holds numbers or NaN, and no byte
    that is no sample written."""
    from bsvd_amd.frame_io import network_size
    f = S.FORMATS[pix_fmt]
    H, W = PAD_PICTURE[f.sub]
    Hp, Wp = network_size(H, W)
    y = _rgb(Hp, Wp, "uniform").copy()
    poisoned = y.copy()
    poisoned[..., H:, :] = np.nan
    poisoned[..., :, W:] = np.nan
    model = []
    for matrix, full_range, chroma in COLOUR:
        kw = dict(matrix=matrix, full_range=full_range, chroma=chroma)
        vals = S.encode_values(y[..., :H, :W], pix_fmt, dtype=np.float64, **kw)
        model.append((kw, vals, [np.abs(v - np.floor(v) - 0.5) <= 1e-3 for v in vals]))
    near, total = sum(int(b.sum()) for _, _, band in model for b in band), sum(b.size for _, _, band in model for b in band)
    assert near <= 0.01 * total, (near, total)
    for kw, vals, band in model:
        for pitches, offsets, stride in _layouts(H, W, pix_fmt):
            stride = stride or S.frame_bytes(H, W, pix_fmt)
            a, big = _encode(y, stride, pix_fmt=pix_fmt, pitches=pitches, offsets=offsets, crop_to=(H, W), **kw)
            b, _ = _encode(poisoned, stride, pix_fmt=pix_fmt, pitches=pitches, offsets=offsets, crop_to=(H, W), **kw)
            assert np.array_equal(a, b), (kw, pitches)
            planes = S.unpack(a, H, W, pix_fmt, pitches, offsets)
            _check_codes(planes, vals, band, (H, W, kw, pitches))
            assert planes[3] == 0
            mask = S.sample_mask(T, H, W, pix_fmt, pitches, offsets, stride)
            assert (a[~mask] == 0xA5).all() and (big[:GUARD] == 0xA5).all() and (big[-GUARD:] == 0xA5).all(), (kw, pitches)


# ---- round trip --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", NAMES)
def test_round_trip_returns_the_codes(pix_fmt):
    """encode(decode(surface)) == surface for 4:4:4 and for chroma='nearest': surfaces made from RGB in uniform(0.4, 0.6), in gamut after
    chroma averaging for every matrix, range and depth."""
    from bsvd_amd.frame_io import output_to_yuv, yuv_to_input
    f = S.FORMATS[pix_fmt]
    H, W = 12, 20
    x = torch.from_numpy((0.4 + _rgb(H, W, "uniform") / 6 + 1 / 60).astype(np.float32)).to("cuda:0")       # (-0.1, 1.1) -> (0.4, 0.6)
    for matrix, full_range in itertools.product(["bt601", "bt709", "bt2020"], [False, True]):
        for chroma in (["nearest", "linear"] if f.sub == 444 else ["nearest"]):
            kw = dict(pix_fmt=pix_fmt, matrix=matrix, full_range=full_range, chroma=chroma)
            e1 = output_to_yuv(x, **kw)
            back = yuv_to_input(e1, H, W, **kw)
            assert 0.0 <= float(back.min()) and float(back.max()) <= 1.0
            assert torch.equal(e1, output_to_yuv(back, **kw)), kw


# ---- the pipelines -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import bsvd_amd
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 11)
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64,
                      pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


PIPE_FORMATS = ["yuv420p", "uyvy422", "yuv444p10le"]
PIPE_SIZE = {None: {420: (32, 48), 422: (32, 48), 444: (32, 48)}, "reflect": {420: (30, 46), 422: (29, 46), 444: (29, 45)}}


def _frames(pix_fmt, n, H, W, seed):
    f = S.FORMATS[pix_fmt]
    dtype = np.uint16 if f.bits > 8 else np.uint8
    return np.random.RandomState(seed).randint(0, 2 ** f.bits, (n, S.frame_bytes(H, W, pix_fmt) // np.dtype(dtype).itemsize)).astype(dtype)


def _direct(m, frames, H, W, pix_fmt, pad):
    """the synchronous path on the same frames: [n, samples] array -> array"""
    from bsvd_amd.frame_io import network_size, output_to_yuv, yuv_to_input
    dev = torch.from_numpy(frames.view(np.uint8).reshape(frames.shape[0], -1)).to("cuda:0")
    y = m.clip_forward(yuv_to_input(dev, H, W, pix_fmt, sigma=SIGMA, pad_to=network_size(H, W) if pad else None))
    return output_to_yuv(y, pix_fmt, crop_to=(H, W) if pad else None).cpu().numpy().view(frames.dtype).reshape(frames.shape)


@pytest.mark.parametrize("pad", [None, "reflect"])
@pytest.mark.parametrize("pix_fmt", PIPE_FORMATS)
def test_live_stream_matches_the_synchronous_path(model, pix_fmt, pad):
    """LiveStream(pix_fmt=..., frame_shape=...): 1-D frames in, 1-D frames out ``latency`` feeds later, byte-identical to
    output_to_yuv(clip_forward(yuv_to_input(frames)))."""
    from bsvd_amd.pipeline import LiveStream
    H, W = PIPE_SIZE[pad][S.FORMATS[pix_fmt].sub]
    live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt=pix_fmt, frame_shape=(H, W), pad=pad)
    assert live.latency == LiveStream(model, sigma=SIGMA, depth=2, frame_shape=(H, W), pad=pad).latency and live.latency_final
    frames = _frames(pix_fmt, live.latency + 2, H, W, 31)
    want = _direct(model, frames, H, W, pix_fmt, pad)
    got = [r for r in (live.feed(fr) for fr in frames) if r is not None]
    assert len(got) == 2
    got += live.flush()
    assert len(got) == len(frames) and all(g.dtype == frames.dtype and g.shape == frames.shape[1:] for g in got)
    assert np.array_equal(np.stack(got), want)
    with pytest.raises(ValueError):
        live.feed(frames[0][:-1])


@pytest.mark.parametrize("pad", [None, "reflect"])
@pytest.mark.parametrize("pix_fmt", PIPE_FORMATS)
def test_clip_pipeline_matches_the_synchronous_path(model, pix_fmt, pad):
    from bsvd_amd.pipeline import ClipPipeline
    H, W = PIPE_SIZE[pad][S.FORMATS[pix_fmt].sub]
    clips = [_frames(pix_fmt, 3 + (i % 2), H, W, 21 + i) for i in range(3)]
    want = [_direct(model, c, H, W, pix_fmt, pad) for c in clips]
    pipe = ClipPipeline(model, sigma=SIGMA, depth=2, pix_fmt=pix_fmt, frame_shape=(H, W), pad=pad)
    got = list(pipe.run(iter(clips)))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    with pytest.raises(ValueError):
        pipe.submit(clips[0][0])


def test_yuv420p_stream_is_the_nv12_stream_reinterleaved(model):
    """the same samples as yuv420p 1-D frames and as NV12 surfaces through two LiveStreams: the same bytes out, after re-interleaving"""
    from bsvd_amd.pipeline import LiveStream
    H, W = 32, 48
    n = 19
    frames = _frames("yuv420p", n, H, W, 41)
    Y, Cb, Cr, _ = S.unpack(frames, H, W, "yuv420p")
    nv12 = M.pack(Y, Cb, Cr, "nv12").reshape(n, H * 3 // 2, W)
    outs = []
    for pix_fmt, fed, kw in (("yuv420p", frames, dict(frame_shape=(H, W))), ("nv12", nv12, {})):
        live = LiveStream(model, sigma=SIGMA, depth=2, pix_fmt=pix_fmt, **kw)
        got = [r for r in (live.feed(fr) for fr in fed) if r is not None] + live.flush()
        assert len(got) == n
        outs.append(np.stack(got))
    y, cb, cr, _ = S.unpack(outs[0], H, W, "yuv420p")
    assert np.array_equal(M.pack(y, cb, cr, "nv12").reshape(n, H * 3 // 2, W), outs[1])
