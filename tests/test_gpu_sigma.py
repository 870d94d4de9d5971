"""The noise-level estimate on the device (bsvd_amd/csrc/frame_sigma.hip through frame_io.estimate_sigma / fill_sigma_plane, the
``sigma='auto'`` of the three ``*_to_input`` functions, ClipPipeline and LiveStream): the histogram equals tests/sigma_model.py's bit for bit
and sigma equals the model's fp32 bit for bit, on every shape at which the kernel takes another path -- one sample per plane, the float4
tails, heights around the row band of an item (sigma_model.BAND = SIGMA_BAND = 8), pictures inside larger tensors with NaN and with finite
values around them, the scalar path -- and on the contents that stress it: a constant frame (every lane on bin 0: the contended path),
a checkerboard (every count in bin 4095), dyadic values on the bin edges, NaN and +-Inf inside the picture, five frames in one call and
the same workspace twice.  End to end: the sigma plane of ``sigma='auto'`` against the model, clip_forward against the host-filled tensor,
the pipelines against the synchronous path byte for byte, LiveStream.last_sigma against the model."""
import numpy as np
import pytest
import torch

import sigma_model as M
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

CASES = M.gpu_cases()
DEV = "cuda:0"


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check(x, picture, gain=1.0, clamp=(0.0, M.SIGMA_MAX)):
    """estimate_sigma on the device against the model: histogram and sigma bit for bit; -> (sigma, hist) of the device"""
    from bsvd_amd.frame_io import estimate_sigma
    d = torch.from_numpy(x).to(DEV)
    s, h = estimate_sigma(d, picture=picture, gain=gain, clamp=clamp, return_hist=True)
    want_s, want_h = M.estimate(x, picture, gain=gain, clamp=clamp)
    got_h = h.cpu().numpy().astype(np.int64)
    assert h.dtype == torch.uint32 and got_h.shape == want_h.shape
    assert np.array_equal(got_h, want_h), "histogram differs in %d bins" % int((got_h != want_h).sum())
    assert s.dtype == torch.float32 and np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)), (s.cpu().numpy(), want_s)
    assert torch.equal(d.cpu(), torch.from_numpy(x)) or np.isnan(x).any()          # the input is only read
    return s, got_h


@pytest.mark.parametrize("name", sorted(CASES))
def test_histogram_and_sigma_equal_the_model_bit_for_bit(name):
    x, picture = CASES[name]
    _check(x, picture)


def test_constant_frame_is_bin_zero_and_checkerboard_the_last_bin():
    """constant: all counts in bin 0, sigma = lo (the contended path).  0 / 1 checkerboard: |r| = 8 at every pixel (16 on a +-1 board):
    all counts in bin 4095, the median in the middle of that bin."""
    x, _ = CASES["constant"]
    s, h = _check(x, None, clamp=(0.01, 0.2))
    n = 3 * 22 * 38
    assert h[0, 0] == n and h[0, 1:].sum() == 0
    assert float(s[0]) == pytest.approx(0.01)                      # med = 0 + N / (2 N) = 0.5 bins: below lo
    x, _ = CASES["checkerboard"]
    s, h = _check(x, None)
    assert h[0, 4095] == n and h[0, :4095].sum() == 0
    assert float(s[0]) == np.float32(4095.5 * M.K)


def test_non_finite_samples_are_not_counted():
    x, _ = CASES["nan_inf"]
    _, h = _check(x, None)
    full = 3 * 22 * 38
    assert (h.sum(1) < full).all() and (h.sum(1) >= full - 9 * 18).all()


def test_nan_outside_the_picture_reaches_no_count_and_the_plane_is_filled():
    """37 x 53 inside 40 x 56: everything outside the picture and the whole sigma plane are NaN before the call"""
    from bsvd_amd.frame_io import estimate_sigma, fill_sigma_plane
    x, picture = CASES["pad_nan_37x53_in_40x56"]
    _, h = _check(x, picture)
    assert (h.sum(1) == 3 * 35 * 51).all()
    d = torch.from_numpy(x).to(DEV)
    s = estimate_sigma(d, picture=picture)
    fill_sigma_plane(d, s)
    got = d.cpu().numpy()
    want = M.estimate(x, picture)[0]
    for t in range(x.shape[0]):
        assert np.array_equal(_bits(got[t, 3]), np.full((40, 56), _bits(want[t])))
    assert np.array_equal(_bits(got[:, :3]), _bits(x[:, :3]))       # the picture planes, NaN pad included, are untouched


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 4, 12, 20), (3, 2, 6, 6)])
def test_fill_writes_the_last_plane_only(shape):
    """scalar stores (35 elements a plane) and float4 stores; the other planes keep their bits"""
    from bsvd_amd.frame_io import fill_sigma_plane
    x = np.random.default_rng(5).uniform(0, 1, shape).astype(np.float32)
    s = np.linspace(0.01, 0.2, shape[0]).astype(np.float32)
    d = torch.from_numpy(x).to(DEV)
    fill_sigma_plane(d, torch.from_numpy(s).to(DEV))
    got = d.cpu().numpy()
    assert np.array_equal(got[:, :-1], x[:, :-1])
    for t in range(shape[0]):
        assert (got[t, -1] == s[t]).all()


def test_gain_and_clamp():
    x, _ = CASES["noisy_three_sigma"]
    _check(x, None, gain=1.37)
    _check(x, None, gain=0.5, clamp=(0.03, 0.05))


def test_same_workspace_twice_and_no_frame_leaks_into_its_neighbour():
    """T = 5 different frames in one call, then other data through the same workspace (the entry point zeroes it itself); each frame's
    histogram is the one it gives alone"""
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    a, b = CASES["five_frames"][0], CASES["five_frames_again"][0]
    T, C, H, W = a.shape
    ws = torch.full((T, 4096), -1, dtype=torch.int32, device=DEV)                  # a dirty workspace
    out = torch.empty(T, dtype=torch.float32, device=DEV)
    assert lib.bsvd_sigma_workspace_bytes(T) == ws.numel() * 4
    stream = torch.cuda.current_stream().cuda_stream
    for x in (a, b, a):
        d = torch.from_numpy(x).to(DEV)
        _lib.check(lib.bsvd_estimate_sigma(d.data_ptr(), T, 3, H, W, H, W, C * H * W, 1.0, 0.0, float(M.SIGMA_MAX), ws.data_ptr(), out.data_ptr(),
                                           stream), "bsvd_estimate_sigma")
        want_s, want_h = M.estimate(x)
        assert np.array_equal(ws.cpu().numpy().view(np.uint32).astype(np.int64), want_h)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want_s))
        for t in range(T):
            assert np.array_equal(M.histogram(x[t:t + 1])[0], want_h[t])
    assert len({float(v) for v in M.estimate(a)[0]}) == T


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """a c32-sized non-blind network"""
    import bsvd_amd
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32), 13)
    m = bsvd_amd.BSVD(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32,
                      pretrain_ckpt=None, precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(torch.device("cuda", 0))


def _rgb_frames(n, H, W, seed):
    sig = [5, 12, 20, 30, 8, 25]
    return np.stack([M.noisy_u8(M.scene("mixed", H, W, seed + t), sig[t % len(sig)], seed + 50 + t).transpose(1, 2, 0) for t in range(n)])


def _host_filled(x0, picture, gain=1.0):
    """x0: the device tensor of the sigma = 0.0 call -> the same tensor with the model's sigma in the plane, filled on the host"""
    ref = x0.cpu().numpy().copy()
    want = M.estimate(ref, picture, gain=gain)[0]
    ref[:, 3] = want[:, None, None]
    return ref, want


def test_frames_to_input_auto_sequence_and_device_tensor(model):
    from bsvd_amd.frame_io import frames_to_input
    H, W = 64, 96
    u8 = torch.from_numpy(_rgb_frames(5, H, W, 7)).to(DEV)
    x0 = frames_to_input(u8, 0.0)
    ref, want = _host_filled(x0, (H, W))
    xa = frames_to_input(u8, "auto")
    assert np.array_equal(_bits(xa.cpu().numpy()), _bits(ref))                    # image planes bit-equal, sigma plane = the model's values
    assert len(set(want.tolist())) == 5 and 3 / 255 < want.min() and want.max() < 33 / 255
    ya = model.clip_forward(xa)
    assert torch.equal(ya, model.clip_forward(torch.from_numpy(ref).to(DEV)))
    assert not torch.equal(ya, model.clip_forward(frames_to_input(u8, 30 / 255.0)))
    ref2, want2 = _host_filled(x0, (H, W), gain=1.25)
    assert np.array_equal(_bits(frames_to_input(u8, "auto", sigma_gain=1.25).cpu().numpy()), _bits(ref2))
    vals = [0.02, 0.05, 0.11, 0.07, 0.03]
    ref3 = x0.cpu().numpy().copy()
    ref3[:, 3] = np.asarray(vals, np.float32)[:, None, None]
    for given in (vals, torch.tensor(vals, dtype=torch.float32, device=DEV)):
        xs = frames_to_input(u8, given)
        assert np.array_equal(_bits(xs.cpu().numpy()), _bits(ref3))
        assert torch.equal(model.clip_forward(xs), model.clip_forward(torch.from_numpy(ref3).to(DEV)))
    with pytest.raises(ValueError):
        frames_to_input(u8, vals[:4])
    assert torch.equal(frames_to_input(u8, 0.1), frames_to_input(u8, [0.1] * 5))   # and a float is what it was


def test_pad_to_estimates_the_picture_not_its_mirror_images():
    from bsvd_amd.frame_io import frames_to_input, network_size
    H, W = 38, 54
    u8 = torch.from_numpy(_rgb_frames(2, H, W, 9)).to(DEV)
    x0 = frames_to_input(u8, 0.0, pad_to=network_size(H, W))
    ref, want = _host_filled(x0, (H, W))
    assert np.array_equal(_bits(frames_to_input(u8, "auto", pad_to=network_size(H, W)).cpu().numpy()), _bits(ref))
    assert not np.array_equal(M.estimate(x0.cpu().numpy(), None)[1], M.estimate(x0.cpu().numpy(), (H, W))[1])


def _yuv_frames(pix_fmt, n, H, W, seed):
    """noisy grey-ish YUV frames: [n, H*3/2, W] (nv12) or [n, samples] (the 1-D formats)"""
    rs = np.random.RandomState(seed)
    if pix_fmt == "nv12":
        return np.clip(rs.normal(128, 12, (n, H * 3 // 2, W)), 16, 235).astype(np.uint8)
    from bsvd_amd.frame_io import yuv_frame_bytes
    return np.clip(rs.normal(128, 12, (n, yuv_frame_bytes(H, W, pix_fmt))), 16, 235).astype(np.uint8)


def _sync(m, frames, pix_fmt, H, W, pad, sigma):
    """the synchronous path on the same frames -> (array like frames, the input tensor's sigma plane values [n])"""
    from bsvd_amd import frame_io as F
    net = F.network_size(H, W) if pad else None
    dev = torch.from_numpy(frames.reshape(frames.shape[0], -1) if pix_fmt != "rgb24" else frames).to(DEV)
    if pix_fmt == "rgb24":
        x = F.frames_to_input(dev, sigma, pad_to=net)
        out = F.output_to_frames(m.clip_forward(x), crop_to=(H, W) if pad else None)
    elif pix_fmt == "nv12":
        x = F.yuv420_to_input(dev, H, W, "nv12", sigma=sigma, pad_to=net)
        out = F.output_to_yuv420(m.clip_forward(x), "nv12", crop_to=(H, W) if pad else None)
    else:
        x = F.yuv_to_input(dev, H, W, pix_fmt, sigma=sigma, pad_to=net)
        out = F.output_to_yuv(m.clip_forward(x), pix_fmt, crop_to=(H, W) if pad else None)
    return out.cpu().numpy().reshape(frames.shape), x[:, 3, 0, 0].cpu().numpy()


PIPE = [("rgb24", None, 64, 96), ("rgb24", "reflect", 38, 54), ("nv12", "reflect", 38, 54), ("yuv422p", "reflect", 38, 54), ("nv12", None, 64, 96)]


def _frames_for(pix_fmt, n, H, W, seed):
    return _rgb_frames(n, H, W, seed) if pix_fmt == "rgb24" else _yuv_frames(pix_fmt, n, H, W, seed)


@pytest.mark.parametrize("pix_fmt,pad,H,W", PIPE)
def test_clip_pipeline_auto_matches_the_synchronous_path(model, pix_fmt, pad, H, W):
    from bsvd_amd.pipeline import ClipPipeline
    clips = [_frames_for(pix_fmt, 3 + (i % 2), H, W, 21 + i) for i in range(3)]
    want = [_sync(model, c, pix_fmt, H, W, pad, "auto")[0] for c in clips]
    kw = {} if pix_fmt in ("rgb24", "nv12") else dict(frame_shape=(H, W))
    pipe = ClipPipeline(model, sigma="auto", depth=2, pix_fmt=pix_fmt, pad=pad, **kw)
    got = list(pipe.run(iter(clips)))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert not np.array_equal(want[0], _sync(model, clips[0], pix_fmt, H, W, pad, 30 / 255.0)[0])


@pytest.mark.parametrize("pix_fmt,pad,H,W", PIPE[:4])
def test_live_stream_auto_matches_the_synchronous_path_and_reports_sigma(model, pix_fmt, pad, H, W):
    """byte-identical to the synchronous path; last_sigma is the estimate of the frame fed depth - 1 calls ago, which is the model's"""
    from bsvd_amd import frame_io as F
    from bsvd_amd.pipeline import LiveStream
    live = LiveStream(model, sigma="auto", depth=2, pix_fmt=pix_fmt, pad=pad, frame_shape=(H, W))
    ref = LiveStream(model, sigma=0.1, depth=2, pix_fmt=pix_fmt, pad=pad, frame_shape=(H, W))
    assert live.latency == ref.latency and live.last_sigma is None
    frames = _frames_for(pix_fmt, live.latency + 3, H, W, 31)
    want, sig = _sync(model, frames, pix_fmt, H, W, pad, "auto")
    if pix_fmt == "rgb24":                                          # ... and those are the model's, on the converted frames
        x0 = F.frames_to_input(torch.from_numpy(frames).to(DEV), 0.0, pad_to=F.network_size(H, W) if pad else None)
        assert np.array_equal(_bits(sig), _bits(M.estimate(x0.cpu().numpy(), (H, W))[0]))
    got = []
    for i, fr in enumerate(frames):
        r = live.feed(fr)
        if r is not None:
            got.append(r)
        if i == 0:
            assert live.last_sigma is None                          # depth 2: the step just fed has not been waited for
        else:
            assert np.float32(live.last_sigma) == sig[i - 1]
    got += live.flush()
    assert np.float32(live.last_sigma) == sig[-1]
    assert len(got) == len(frames) and np.array_equal(np.stack(got), want)
