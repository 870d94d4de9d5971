"""YUV 4:2:0 frame I/O on the device (bsvd_amd/csrc/frame_yuv.hip through frame_io.yuv420_to_input / output_to_yuv420 and the pipelines'
pix_fmt) against the independent numpy model tests/yuv_model.py.  Sizes are the smallest at which the kernels' item map (4 columns x 2
rows per lane) can go wrong: 4x4 is one item, 8x12 an odd item count per row, 36x52 has row and column tails in any wider item grid,
64x96 is the pipelines' test size; one and three frames; tight surfaces and pitched ones with gaps between the frames."""
import functools
import itertools

import numpy as np
import pytest
import torch

import yuv_model as M
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

SIZES = [(4, 4), (8, 12), (36, 52), (64, 96)]
FRAMES = [1, 3]
CONFIGS = list(itertools.product(["nv12", "p010"], ["bt601", "bt709", "bt2020"], [False, True], ["nearest", "linear"]))
GUARD = 66          # bytes in front of a surface inside its allocation: surfaces promise no more than their sample's alignment
SIGMA = 30 / 255.0


def _layouts(H, W, pix_fmt):
    """(row_pitch, frame_stride) in bytes: tight, and rows rounded up to 64 bytes plus 64 with frames one frame plus 128 apart"""
    tight = W * (2 if pix_fmt == "p010" else 1)
    pitch = (tight + 63) // 64 * 64 + 64
    return [(None, None), (pitch, pitch * H * 3 // 2 + 128)]


@functools.lru_cache(maxsize=None)
def _codes(pix_fmt, T, H, W):
    """seeded random codes over the full code range (+ junk for the low 6 bits of P010 words); shared, never written"""
    rs = np.random.RandomState(1000 * T + 10 * H + W)
    top = 2 ** M.BITS[pix_fmt]
    out = (rs.randint(0, top, (T, H, W)), rs.randint(0, top, (T, H // 2, W // 2)), rs.randint(0, top, (T, H // 2, W // 2)),
           rs.randint(0, 64, (T, H * 3 // 2, W)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _rgb(T, H, W, lo, hi):
    return np.random.RandomState(7 * T + 3 * H + W).uniform(lo, hi, (T, 3, H, W)).astype(np.float32)       # shared, never written


def _surface(buf, fill):
    """host surface [T, stride] -> device view of the same bytes inside a larger allocation filled with ``fill``"""
    T, stride = buf.shape
    big = torch.full((GUARD + T * stride + GUARD,), fill, dtype=torch.uint8, device="cuda:0")
    view = big[GUARD:GUARD + T * stride].view(T, stride)
    view.copy_(torch.from_numpy(buf))
    return big, view


def _decode(buf, H, W, fill=0xFF, **kw):
    from bsvd_amd.frame_io import yuv420_to_input
    _, view = _surface(buf, fill)
    return yuv420_to_input(view, H, W, **kw).cpu().numpy()


def _encode(x, stride, **kw):
    """-> (the surface [T, stride], the whole allocation around it) after an encode into memory prefilled with 0xA5"""
    from bsvd_amd.frame_io import output_to_yuv420
    big, view = _surface(np.full((x.shape[0], stride), 0xA5, np.uint8), 0xA5)
    got = output_to_yuv420(torch.from_numpy(x).to("cuda:0"), out=view, **kw)
    assert got.data_ptr() == view.data_ptr()
    return view.cpu().numpy(), big.cpu().numpy()


@pytest.mark.parametrize("pix_fmt,matrix,full_range,chroma", CONFIGS)
def test_decode_matches_the_float64_model(pix_fmt, matrix, full_range, chroma):
    """max-abs <= 1e-6 on values of O(1): the float32 model differs from the float64 one by 1.4e-7 on these inputs and a conforming kernel
    may associate its FMAs differently, hence the factor 7.  Random codes over the full code range, P010 words with random low 6 bits
    (ignored); the sigma channel is bit-equal to float32(sigma); a surface whose padding, gaps and surroundings hold 0xFF bytes decodes to
    the bits of the tight one."""
    bits = M.BITS[pix_fmt]
    kw = dict(pix_fmt=pix_fmt, matrix=matrix, full_range=full_range, chroma=chroma)
    worst = 0.0
    for (H, W), T in itertools.product(SIZES, FRAMES):
        Y, Cb, Cr, low = _codes(pix_fmt, T, H, W)
        want = M.decode(Y, Cb, Cr, bits, matrix=matrix, full_range=full_range, chroma=chroma, dtype=np.float64)
        results = []
        for pitch, stride in _layouts(H, W, pix_fmt):
            buf = M.pack(Y, Cb, Cr, pix_fmt, pitch, stride, fill=0xFF, low_bits=low)
            got = _decode(buf, H, W, sigma=SIGMA, row_pitch=pitch, **kw)
            assert got.shape == (T, 4, H, W) and got.dtype == np.float32
            assert (got[:, 3].view(np.uint32) == np.float32(SIGMA).view(np.uint32)).all()
            err = float(np.abs(got[:, :3].astype(np.float64) - want).max())
            worst = max(worst, err)
            assert err <= 1e-6, (H, W, T, pitch, err)
            results.append(got)
        assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32)), (H, W, T)
        blind = _decode(M.pack(Y, Cb, Cr, pix_fmt, low_bits=low), H, W, **kw)                       # no sigma: three channels
        assert blind.shape == (T, 3, H, W) and np.array_equal(blind.view(np.uint32), results[0][:, :3].view(np.uint32))
    print("decode %s %s full_range=%s %s: max-abs vs float64 model %.3e" % (pix_fmt, matrix, full_range, chroma, worst))


@pytest.mark.parametrize("pix_fmt,matrix,full_range,chroma", CONFIGS)
def test_encode_matches_the_float64_model(pix_fmt, matrix, full_range, chroma):
    """Codes equal rint of the float64 model except where its pre-rounding value lies within 1e-3 of a half-integer (there +-1 is accepted);
    such samples are at most 1 % of the case's samples (the model alone puts <= 0.36 % there on these inputs).  P010 low 6 bits are zero.
    Guard bytes around the surface, pitch padding and the gaps between frames keep their 0xA5."""
    bits = M.BITS[pix_fmt]
    kw = dict(pix_fmt=pix_fmt, matrix=matrix, full_range=full_range, chroma=chroma)
    near = total = 0
    for (H, W), T in itertools.product(SIZES, FRAMES):
        x = _rgb(T, H, W, -0.1, 1.1)
        vals = M.encode_values(x, bits, matrix=matrix, full_range=full_range, chroma=chroma, dtype=np.float64)
        band = [np.abs(v - np.floor(v) - 0.5) <= 1e-3 for v in vals]
        near += sum(int(b.sum()) for b in band)
        total += sum(b.size for b in band)
        for pitch, stride in _layouts(H, W, pix_fmt):
            stride = stride or M.frame_bytes(H, W, pix_fmt)
            surf, big = _encode(x, stride, row_pitch=pitch, **kw)
            planes = M.unpack(surf, H, W, pix_fmt, pitch)
            for name, got, v, b in zip("Y Cb Cr".split(), planes, vals, band):
                d = got - np.rint(v).astype(np.int64)
                bad = (d != 0) & ~(b & (np.abs(d) == 1))
                assert not bad.any(), (H, W, T, pitch, name, int(bad.sum()), got[bad][:4], v[bad][:4])
            if pix_fmt == "p010":
                assert (planes[3] & 63 == 0).all()
            mask = M.sample_mask(T, H, W, pix_fmt, pitch, stride)
            assert (surf[~mask] == 0xA5).all(), (H, W, T, pitch)
            assert (big[:GUARD] == 0xA5).all() and (big[-GUARD:] == 0xA5).all(), (H, W, T, pitch)
    print("encode %s %s full_range=%s %s: %d of %d samples within 1e-3 of a half-integer" % (pix_fmt, matrix, full_range, chroma, near, total))
    assert near <= 0.01 * total


def test_output_without_out_allocates_a_zero_padded_surface():
    from bsvd_amd.frame_io import output_to_yuv420, yuv420_frame_bytes
    x = torch.from_numpy(_rgb(3, 36, 52, -0.1, 1.1)).to("cuda:0")
    for pix_fmt, pitch in (("nv12", None), ("nv12", 128), ("p010", 192)):
        got = output_to_yuv420(x, pix_fmt=pix_fmt, row_pitch=pitch)
        assert got.shape == (3, yuv420_frame_bytes(36, 52, pix_fmt, pitch)) and got.dtype == torch.uint8
        surf, _ = _encode(x.cpu().numpy(), got.shape[1], pix_fmt=pix_fmt, row_pitch=pitch)
        mask = M.sample_mask(3, 36, 52, pix_fmt, pitch)
        got = got.cpu().numpy()
        assert np.array_equal(got[mask], surf[mask]) and (got[~mask] == 0).all()


@pytest.mark.parametrize("pix_fmt", ["nv12", "p010"])
def test_round_trip_is_a_fixed_point(pix_fmt):
    """chroma='nearest', RGB from uniform(0.4, 0.6) -- in gamut after chroma averaging for every matrix, range and depth --:
    encode(decode(encode(x))) is byte-identical to encode(x)."""
    from bsvd_amd.frame_io import output_to_yuv420, yuv420_to_input
    for (H, W), matrix, full_range in itertools.product([(36, 52), (64, 96)], ["bt601", "bt709", "bt2020"], [False, True]):
        kw = dict(pix_fmt=pix_fmt, matrix=matrix, full_range=full_range, chroma="nearest")
        x = torch.from_numpy(_rgb(3, H, W, 0.4, 0.6)).to("cuda:0")
        e1 = output_to_yuv420(x, **kw)
        back = yuv420_to_input(e1, H, W, **kw)
        assert 0.0 <= float(back.min()) and float(back.max()) <= 1.0
        e2 = output_to_yuv420(back, **kw)
        assert torch.equal(e1, e2), (H, W, matrix, full_range)


# ---- the pipelines: tests/test_gpu_eval.py's two pipeline tests with YUV surfaces, same seeded model ------------------------------------------
@pytest.fixture(scope="module")
def model():
    import bsvd_amd
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 11)
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64,
                      pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


def _direct(m, frames, H, W, pix_fmt, row_pitch=None):
    """the synchronous path on the same surfaces: [T, H*3/2, pitch] array -> array"""
    from bsvd_amd.frame_io import output_to_yuv420, yuv420_to_input
    dev = torch.from_numpy(frames.view(np.uint8).reshape(frames.shape[0], -1)).to("cuda:0")
    y = m.clip_forward(yuv420_to_input(dev, H, W, pix_fmt, sigma=SIGMA, row_pitch=row_pitch))
    return output_to_yuv420(y, pix_fmt, row_pitch=row_pitch).cpu().numpy().view(frames.dtype).reshape(frames.shape)


@pytest.mark.parametrize("pix_fmt,depth,pitched", [("nv12", 1, False), ("nv12", 2, False), ("p010", 2, True)])
def test_live_stream_yuv_frames_match_the_clip_path(model, pix_fmt, depth, pitched):
    """LiveStream(pix_fmt=...): surfaces in, surfaces out ``latency`` feeds later -- the latency of 'rgb24' --, byte-identical to
    output_to_yuv420(clip_forward(yuv420_to_input(frames))); reusable after flush()."""
    from bsvd_amd.pipeline import LiveStream
    m = model
    H, W = 64, 96
    dtype, top = (np.uint8, 256) if pix_fmt == "nv12" else (np.uint16, 65536)
    pitch = 128 if pitched else W                                    # samples
    colour = {"row_pitch": pitch * np.dtype(dtype).itemsize, "width": W} if pitched else None
    rs = np.random.RandomState(31)
    live = LiveStream(m, sigma=SIGMA, depth=depth, pix_fmt=pix_fmt, colour=colour)
    assert live.overlap == (depth >= 2)
    assert live.latency == m.shift_num + depth - 1 + (1 if live.overlap else 0)
    assert live.latency == LiveStream(m, sigma=SIGMA, depth=depth).latency
    for T in (23, 5):
        frames = rs.randint(0, top, (T, H * 3 // 2, pitch)).astype(dtype)
        want = _direct(m, frames, H, W, pix_fmt, colour["row_pitch"] if pitched else None)
        got, first = [], None
        for k in range(T):
            r = live.feed(frames[k])
            if r is not None:
                first = k if first is None else first
                got.append(r)
        if T > live.latency:
            assert first == live.latency
        got += live.flush()
        assert len(got) == T and all(g.dtype == dtype and g.shape == frames.shape[1:] for g in got)
        assert np.array_equal(np.stack(got), want)
    with pytest.raises(ValueError):
        live.feed(np.zeros((H * 3 // 2, pitch), np.float32))
    with pytest.raises(ValueError):
        live.feed(np.zeros((H, W, 3), np.uint8))


def test_clip_pipeline_nv12_matches_the_direct_path(model):
    """ClipPipeline(pix_fmt='nv12') over clips of alternating length, depth 2: in order, the bytes of the synchronous path."""
    from bsvd_amd.pipeline import ClipPipeline
    m = model
    H, W = 64, 96
    rs = np.random.RandomState(21)
    clips = [rs.randint(0, 256, (3 + (i % 2), H * 3 // 2, W)).astype(np.uint8) for i in range(5)]
    want = [_direct(m, c, H, W, "nv12") for c in clips]
    pipe = ClipPipeline(m, sigma=SIGMA, depth=2, pix_fmt="nv12")
    got = list(pipe.run(iter(clips)))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)
    with pytest.raises(ValueError):
        pipe.submit(np.zeros((2, H * 3 // 2, W), np.uint16))
