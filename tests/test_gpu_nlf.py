"""The noise-level function on the device (bsvd_amd/csrc/frame_nlf.hip through frame_io.estimate_noise_curve / noise_curve_from_hist /
fill_noise_map, the ``sigma='nlf'`` and ``sigma=NoiseCurve`` of the ``*_to_input`` functions, ClipPipeline and LiveStream): histogram
[T,16,1024], curve and map equal tests/nlf_model.py's bit for bit on the shapes and contents at which the kernels take another path; the
level-summed histogram equals the scalar estimator's; the map pass writes its plane, all of it and nothing else; the curve rules on hand-built
histograms; end to end against the steps done by hand and the pipelines against the synchronous path byte for byte.  The modes that existed
before give the digests profiles/noise_curve.txt records from the commit before this one."""
import numpy as np
import pytest
import torch

import nlf_defaults
import nlf_model as M
import sigma_model as S

pytestmark = pytest.mark.gpu

CASES = M.gpu_cases()
CURVES = M.curve_cases()
DEV = "cuda:0"


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(x, picture, **kw):
    """estimate_noise_curve and fill_noise_map on the device against the model: histogram, curve and map bit for bit -> (curve, hist) of the device"""
    from bsvd_amd.frame_io import estimate_noise_curve, fill_noise_map
    d = torch.from_numpy(x).to(DEV)
    c, h = estimate_noise_curve(d, picture=picture, return_hist=True, **kw)
    mk = dict(kw)
    if "clamp" in mk:
        mk["clamp"] = tuple(mk["clamp"])
    want_c, want_h = M.estimate(x, picture, **mk)
    got_h = h.cpu().numpy().astype(np.int64)
    assert h.dtype == torch.uint32 and got_h.shape == want_h.shape
    assert np.array_equal(got_h, want_h), "histogram differs in %d entries" % int((got_h != want_h).sum())
    got_c = c.cpu().numpy()
    assert c.dtype == torch.float32 and np.array_equal(_bits(got_c), _bits(want_c)), (got_c, want_c)
    d[:, 3] = float("nan")
    fill_noise_map(d, c)
    got = d.cpu().numpy()
    assert np.array_equal(_bits(got[:, 3]), _bits(M.noise_map(x, want_c)))
    assert np.array_equal(_bits(got[:, :3]), _bits(x[:, :3]))                    # the colour planes are only read
    assert np.isfinite(got[:, 3]).all()
    return got_c, got_h


@pytest.mark.parametrize("name", sorted(CASES))
def test_histogram_curve_and_map_equal_the_model_bit_for_bit(name):
    x, picture = CASES[name]
    _check(x, picture)


def test_flat_frame_is_one_entry_and_the_checkerboard_two_levels():
    """flat: every lane of every wave on one (level, bin), the contended path.  0.25 / 0.75 checkerboard: |r| = 4, the last bin of two levels."""
    n = 3 * 22 * 38
    _, h = _check(CASES["flat"][0], None, min_count=1)
    assert h[0, 8, 0] == n and h.sum() == n
    _, h = _check(CASES["checkerboard"][0], None, min_count=1)
    assert h[0, 7, 1023] + h[0, 8, 1023] == n and h[0, 7, 1023] > 0 and h[0, 8, 1023] > 0


def test_nan_outside_the_picture_reaches_no_count_and_non_finite_samples_are_not_counted():
    x, picture = CASES["pad_nan_37x50_in_40x52"]
    assert np.isnan(x[:, :, 37:]).all() and np.isnan(x[:, :, :, 50:]).all()
    _, h = _check(x, picture)
    assert (h.sum((1, 2)) == 3 * 35 * 48).all()
    _, h = _check(CASES["nan_inf"][0], None)
    full = 3 * 22 * 38
    assert (h.sum((1, 2)) < full).all() and (h.sum((1, 2)) >= full - 9 * 18).all()


def test_gain_clamp_and_min_count():
    x, _ = CASES["noisy_5x64x96"]
    _check(x, None, gain=1.37)
    _check(x, None, gain=0.5, clamp=(0.02, 0.03))
    _check(x, None, min_count=1)
    _check(x, None, min_count=3000)


def test_base_pointer_offset_by_one_float_takes_the_scalar_path():
    """the raw ABI on a frame that starts one float behind a 16-byte boundary: histogram, curve and map are the aligned call's"""
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    x, _ = CASES["noisy_1x64x96"]
    T, C, H, W = x.shape
    want_c, want_h = M.estimate(x)
    buf = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device=DEV)
    buf[1:1 + x.size] = torch.from_numpy(x).reshape(-1).to(DEV)
    ws = torch.full((T, 16, 1024), -1, dtype=torch.int32, device=DEV)
    out = torch.empty((T, 16), dtype=torch.float32, device=DEV)
    ptr = buf.data_ptr() + 4
    assert buf.data_ptr() % 16 == 0
    _lib.check(lib.bsvd_estimate_nlf(ptr, T, H, W, H, W, C * H * W, 1.0, 0.0, float(M.SIGMA_MAX), 512, ws.data_ptr(), out.data_ptr(), _stream()),
               "bsvd_estimate_nlf")
    assert np.array_equal(ws.cpu().numpy().view(np.uint32).astype(np.int64), want_h)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want_c))
    _lib.check(lib.bsvd_fill_nlf_plane(ptr, T, 3, H, W, C * H * W, out.data_ptr(), _stream()), "bsvd_fill_nlf_plane")
    got = buf.cpu().numpy()
    assert np.array_equal(_bits(got[1:1 + x.size].reshape(x.shape)[:, 3]), _bits(M.noise_map(x, want_c)))
    assert np.array_equal(_bits(got[1:1 + x.size].reshape(x.shape)[:, :3]), _bits(x[:, :3]))
    assert np.isnan(got[0]) and np.isnan(got[1 + x.size:]).all()


def test_one_frame_and_sixty_four_frames_have_identical_counts():
    """T = 1 and T = 64 run with different grid caps: integer counts do not depend on the launch shape"""
    from bsvd_amd.frame_io import estimate_noise_curve
    x, _ = CASES["noisy_1x64x96"]
    d = torch.from_numpy(x).to(DEV)
    c1, h1 = estimate_noise_curve(d, return_hist=True)
    c64, h64 = estimate_noise_curve(d.expand(64, -1, -1, -1).contiguous(), return_hist=True)
    assert torch.equal(h64.view(torch.int32), h1.view(torch.int32).expand(64, -1, -1))
    assert torch.equal(c64.view(torch.int32), c1.view(torch.int32).expand(64, -1))


@pytest.mark.parametrize("name", ["noisy_5x64x96", "pad_nan_37x50_in_40x52", "scalar_11x67", "nan_inf"])
def test_level_summed_histogram_equals_the_scalar_estimator_s_in_fours(name):
    from bsvd_amd.frame_io import estimate_noise_curve, estimate_sigma
    x, picture = CASES[name]
    d = torch.from_numpy(x).to(DEV)
    _, h = estimate_noise_curve(d, picture=picture, return_hist=True)
    _, hs = estimate_sigma(d, picture=picture, return_hist=True)
    got = h.cpu().numpy().astype(np.int64).sum(1)
    assert np.array_equal(got, hs.cpu().numpy().astype(np.int64).reshape(x.shape[0], 1024, 4).sum(2))


# ---- the map pass ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 4, 12, 20), (3, 5, 6, 6), (2, 4, 40, 52)])
def test_constant_curve_gives_the_bytes_of_fill_sigma_plane(shape):
    """scalar and float4 stores; the other planes keep their bits; every element of the map plane is written, starting from NaN"""
    from bsvd_amd.frame_io import fill_noise_map, fill_sigma_plane
    x = np.random.default_rng(5).uniform(-0.2, 1.2, shape).astype(np.float32)
    x[:, -1] = np.nan
    s = np.linspace(0.01, 0.2, shape[0]).astype(np.float32)
    a, b = torch.from_numpy(x).to(DEV), torch.from_numpy(x).to(DEV)
    fill_sigma_plane(a, torch.from_numpy(s).to(DEV))
    fill_noise_map(b, torch.from_numpy(np.repeat(s[:, None], 16, 1)).to(DEV))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(_bits(b.cpu().numpy()[:, :-1]), _bits(x[:, :-1]))


@pytest.mark.parametrize("offset", [64, 61])
def test_map_writes_nothing_outside_its_plane_inside_a_poisoned_arena(offset):
    """the frames sit `offset` floats into an arena of sentinels (61: the scalar path), two frames a stride of 5 planes apart with 4 in use"""
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    x, _ = CASES["shape_2x12x20"]
    T, C, H, W = x.shape
    stride = 5 * H * W
    c = M.estimate(x)[0]
    sentinel = np.float32(-77.25)
    arena = np.full(offset + T * stride + 64, sentinel, np.float32)
    for t in range(T):
        arena[offset + t * stride: offset + t * stride + 3 * H * W] = x[t, :3].reshape(-1)
    d = torch.from_numpy(arena).to(DEV)
    cd = torch.from_numpy(c).to(DEV)
    _lib.check(lib.bsvd_fill_nlf_plane(d.data_ptr() + 4 * offset, T, 3, H, W, stride, cd.data_ptr(), _stream()), "bsvd_fill_nlf_plane")
    got = d.cpu().numpy()
    want = arena.copy()
    m = M.noise_map(x, c)
    for t in range(T):
        want[offset + t * stride + 3 * H * W: offset + t * stride + 4 * H * W] = m[t].reshape(-1)
    assert np.array_equal(_bits(got), _bits(want))


def test_same_workspace_twice_and_no_frame_leaks_into_its_neighbour():
    """T = 5 different frames in one call, then other data through the same dirty workspace (the entry point zeroes it itself); each frame's
    histogram, curve and map are the ones it gives alone"""
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    a = CASES["noisy_5x64x96"][0]
    b = a[::-1].copy()
    T, C, H, W = a.shape
    ws = torch.full((T, 16, 1024), -1, dtype=torch.int32, device=DEV)
    out = torch.empty((T, 16), dtype=torch.float32, device=DEV)
    assert lib.bsvd_nlf_workspace_bytes(T) == ws.numel() * 4
    alone = [M.estimate(a[t:t + 1]) for t in range(T)]
    for x in (a, b, a):
        d = torch.from_numpy(x).to(DEV)
        _lib.check(lib.bsvd_estimate_nlf(d.data_ptr(), T, H, W, H, W, C * H * W, 1.0, 0.0, float(M.SIGMA_MAX), 512, ws.data_ptr(), out.data_ptr(),
                                         _stream()), "bsvd_estimate_nlf")
        _lib.check(lib.bsvd_fill_nlf_plane(d.data_ptr(), T, 3, H, W, C * H * W, out.data_ptr(), _stream()), "bsvd_fill_nlf_plane")
        order = range(T) if x is a else range(T - 1, -1, -1)
        got_h, got_c, got_m = ws.cpu().numpy().view(np.uint32).astype(np.int64), out.cpu().numpy(), d.cpu().numpy()[:, 3]
        for t, src in enumerate(order):
            assert np.array_equal(got_h[t], alone[src][1][0]) and np.array_equal(_bits(got_c[t]), _bits(alone[src][0][0]))
            assert np.array_equal(_bits(got_m[t]), _bits(M.noise_map(a[src:src + 1], alone[src][0])[0]))
    assert len({tuple(c[0].tolist()) for c, _ in alone}) == T


# ---- the curve rules, on hand-built histograms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CURVES))
def test_curve_rules_on_hand_built_histograms(name):
    """min_count boundary, nearest-valid fill with a tie, no valid level -> pooled, empty -> lo, gain and clamp: the finish alone"""
    from bsvd_amd.frame_io import noise_curve_from_hist
    h, kw = CURVES[name]
    d = torch.from_numpy(h.astype(np.int32)).to(DEV).view(torch.uint32)
    args = dict(gain=kw.get("gain", 1.0), clamp=(kw.get("lo", 0.0), kw.get("hi", M.SIGMA_MAX)), min_count=kw.get("min_count", 512))
    got = noise_curve_from_hist(d, **args).cpu().numpy()
    assert got.shape == (h.shape[0], 16) and np.array_equal(_bits(got), _bits(M.curve(h, **kw)))
    assert torch.equal(d.view(torch.int32).cpu(), torch.from_numpy(h.astype(np.int32)))      # the histograms are only read
    if name == "min_count_boundary":
        assert got[0, 4] == got[0, 3] == np.float32(10.5 * M.K)
        assert noise_curve_from_hist(d, min_count=99).cpu().numpy()[0, 4] == np.float32(50.5 * M.K)
    if name == "tie_to_the_lower_level":
        assert got[0].tolist() == [np.float32(20.5 * M.K)] * 5 + [np.float32(80.5 * M.K)] * 11
    if name == "empty_gives_lo":
        assert (got == np.float32(0.0125)).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return nlf_defaults.small_model()


def _pg_frames(n, H, W, seed):
    """uint8 RGB frames [n, H, W, 3] with signal-dependent noise"""
    return np.stack([M.poisson_gauss_u8(S.scene("mixed", H, W, seed + t), seed + 50 + t, a=M.A * (1 + t % 3)).transpose(1, 2, 0) for t in range(n)])


def _yuv_frames(pix_fmt, n, H, W, seed):
    rs = np.random.RandomState(seed)
    from bsvd_amd.frame_io import yuv_frame_bytes
    shape = (n, H * 3 // 2, W) if pix_fmt == "nv12" else (n, yuv_frame_bytes(H, W, pix_fmt))
    return np.clip(rs.normal(128, 12, shape) + np.linspace(-60, 60, shape[-1]), 16, 235).astype(np.uint8)


def _by_hand(x0, picture, gain=1.0):
    """x0: the tensor of the sigma = 0.0 call -> conversion + estimate_noise_curve(picture=) + fill_noise_map by hand, and the curve"""
    from bsvd_amd.frame_io import estimate_noise_curve, fill_noise_map
    c = estimate_noise_curve(x0, picture=picture, gain=gain)
    return fill_noise_map(x0.clone(), c), c


def test_frames_to_input_nlf_and_a_given_curve(model):
    from bsvd_amd.frame_io import NoiseCurve, fill_noise_map, frames_to_input
    H, W = 64, 96
    u8 = torch.from_numpy(_pg_frames(5, H, W, 7)).to(DEV)
    x0 = frames_to_input(u8, 0.0)
    want, c = _by_hand(x0, (H, W))
    xn = frames_to_input(u8, "nlf")
    assert torch.equal(xn.view(torch.int32), want.view(torch.int32))
    ref = x0.cpu().numpy()
    mc = M.estimate(ref, (H, W))[0]                                               # ... and both are the model's
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(mc)) and np.array_equal(_bits(xn[:, 3].cpu().numpy()), _bits(M.noise_map(ref, mc)))
    plane = xn[:, 3].cpu().numpy()
    assert (plane.max((1, 2)) > 1.3 * plane.min((1, 2))).all()                    # a map, not a constant
    assert not torch.equal(model.clip_forward(xn), model.clip_forward(frames_to_input(u8, "auto")))
    want2, _ = _by_hand(x0, (H, W), gain=1.25)
    assert torch.equal(frames_to_input(u8, "nlf", sigma_gain=1.25).view(torch.int32), want2.view(torch.int32))
    given = NoiseCurve.from_model(M.A, M.B)
    cg = torch.tensor(given.values, dtype=torch.float32, device=DEV).expand(5, 16).contiguous()
    assert torch.equal(frames_to_input(u8, given).view(torch.int32), fill_noise_map(x0.clone(), cg).view(torch.int32))
    assert torch.equal(frames_to_input(u8, NoiseCurve([0.1] * 16)), frames_to_input(u8, 0.1))       # a flat curve is the constant plane


def test_yuv_and_rgb_to_input_nlf_equal_the_steps_by_hand():
    from bsvd_amd import frame_io as F
    H, W = 38, 54
    net = F.network_size(H, W)
    buf = torch.from_numpy(_yuv_frames("yuv422p", 3, H, W, 11)).to(DEV)
    x0 = F.yuv_to_input(buf, H, W, "yuv422p", sigma=0.0, pad_to=net)
    want, _ = _by_hand(x0, (H, W))
    got = F.yuv_to_input(buf, H, W, "yuv422p", sigma="nlf", pad_to=net)
    assert got.shape == (3, 4) + net and torch.equal(got.view(torch.int32), want.view(torch.int32))
    full, _ = _by_hand(x0, None)                                                  # the mirror images are not sampled
    assert not torch.equal(full.view(torch.int32), want.view(torch.int32))
    nv = torch.from_numpy(_yuv_frames("nv12", 2, H, W, 12).reshape(2, -1)).to(DEV)
    x0 = F.yuv420_to_input(nv, H, W, "nv12", sigma=0.0, pad_to=net)
    assert torch.equal(F.yuv420_to_input(nv, H, W, "nv12", sigma="nlf", pad_to=net).view(torch.int32), _by_hand(x0, (H, W))[0].view(torch.int32))
    rs = np.random.RandomState(13)
    bgra = torch.from_numpy(np.clip(rs.normal(128, 12, (2, F.rgb_frame_bytes(H, W, "bgra"))) + np.linspace(-70, 70, F.rgb_frame_bytes(H, W, "bgra")),
                                    0, 255).astype(np.uint8)).to(DEV)
    x0 = F.rgb_to_input(bgra, H, W, "bgra", sigma=0.0, pad_to=net)
    got = F.rgb_to_input(bgra, H, W, "bgra", sigma="nlf", pad_to=net, sigma_gain=0.8)
    assert torch.equal(got.view(torch.int32), _by_hand(x0, (H, W), gain=0.8)[0].view(torch.int32))


def _sync(m, frames, pix_fmt, H, W, pad, sigma):
    """the synchronous path on the same frames -> (array like frames, the device curves [n, 16])"""
    from bsvd_amd import frame_io as F
    net = F.network_size(H, W) if pad else None
    dev = torch.from_numpy(frames.reshape(frames.shape[0], -1) if pix_fmt != "rgb24" else frames).to(DEV)
    if pix_fmt == "rgb24":
        x = F.frames_to_input(dev, sigma, pad_to=net)
        out = F.output_to_frames(m.clip_forward(x), crop_to=(H, W) if pad else None)
    else:
        x = F.yuv420_to_input(dev, H, W, "nv12", sigma=sigma, pad_to=net)
        out = F.output_to_yuv420(m.clip_forward(x), "nv12", crop_to=(H, W) if pad else None)
    return out.cpu().numpy().reshape(frames.shape), F.estimate_noise_curve(x, picture=(H, W)).cpu().numpy()


PIPE = [("rgb24", None, 64, 96), ("rgb24", "reflect", 38, 54), ("nv12", None, 64, 96), ("nv12", "reflect", 38, 54)]


def _frames_for(pix_fmt, n, H, W, seed):
    return _pg_frames(n, H, W, seed) if pix_fmt == "rgb24" else _yuv_frames(pix_fmt, n, H, W, seed)


@pytest.mark.parametrize("pix_fmt,pad,H,W", PIPE)
def test_clip_pipeline_nlf_matches_the_synchronous_path(model, pix_fmt, pad, H, W):
    from bsvd_amd.frame_io import NoiseCurve
    from bsvd_amd.pipeline import ClipPipeline
    clips = [_frames_for(pix_fmt, 3 + (i % 2), H, W, 21 + i) for i in range(3)]
    for sigma in ("nlf", NoiseCurve.from_model(M.A, M.B)):
        want = [_sync(model, c, pix_fmt, H, W, pad, sigma)[0] for c in clips]
        got = list(ClipPipeline(model, sigma=sigma, depth=2, pix_fmt=pix_fmt, pad=pad).run(iter(clips)))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert not np.array_equal(want[0], _sync(model, clips[0], pix_fmt, H, W, pad, "auto")[0])


@pytest.mark.parametrize("pix_fmt,pad,H,W", PIPE)
def test_live_stream_nlf_matches_the_synchronous_path_and_reports_the_curve(model, pix_fmt, pad, H, W):
    """byte-identical to the synchronous path; last_noise_curve is the device curve of the frame fed depth - 1 calls ago; last_sigma stays None"""
    from bsvd_amd.pipeline import LiveStream
    live = LiveStream(model, sigma="nlf", depth=2, pix_fmt=pix_fmt, pad=pad, frame_shape=(H, W))
    assert live.last_noise_curve is None and live.last_sigma is None and not live.auto_sigma
    frames = _frames_for(pix_fmt, live.latency + 3, H, W, 31)
    want, curves = _sync(model, frames, pix_fmt, H, W, pad, "nlf")
    got = []
    for i, fr in enumerate(frames):
        r = live.feed(fr)
        if r is not None:
            got.append(r)
        if i == 0:
            assert live.last_noise_curve is None
        else:
            assert len(live.last_noise_curve) == 16 and np.array_equal(_bits(live.last_noise_curve), _bits(curves[i - 1]))
    got += live.flush()
    assert np.array_equal(_bits(live.last_noise_curve), _bits(curves[-1])) and live.last_sigma is None
    assert len(got) == len(frames) and np.array_equal(np.stack(got), want)


def test_live_stream_nlf_steady_state_allocates_nothing_and_captures_no_new_graph(model):
    from bsvd_amd.pipeline import LiveStream
    H, W = 64, 96
    live = LiveStream(model, sigma="nlf", depth=2, frame_shape=(H, W))
    frames = _pg_frames(6, H, W, 41)
    from bsvd_amd.stream_plan import RING_PERIOD
    warm = live.latency + 2 * RING_PERIOD + 2                                     # fill, first sightings (batched launches), second (captures)
    for i in range(warm):
        live.feed(frames[i % 6])
    caps, replays = model._stream_eng.stats["graph_captures"], model._stream_eng.stats["graph_replays"]
    mem = []
    for i in range(RING_PERIOD + 2):
        assert live.feed(frames[i % 6]) is not None
        mem.append(torch.cuda.memory_allocated())
    assert len(set(mem)) == 1, ("device memory moved between feeds", mem)
    assert model._stream_eng.stats["graph_captures"] == caps and model._stream_eng.stats["graph_replays"] > replays
    live.flush()


def test_the_modes_that_existed_before_give_the_recorded_digests(model):
    """sigma = 30 / 255 and sigma = 'auto' through frames_to_input, clip_forward, ClipPipeline and LiveStream: the digests recorded from the
    commit before the noise-level function (profiles/noise_curve.txt, section 5), not recomputed by the code under test"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "noise_curve.txt")).read()
    recorded = dict(re.findall(r'^ "([0-9x]+ [A-Za-z]+ [a-z0-9]+)": "([0-9a-f]{16})"', text, re.M))
    assert len(recorded) == 16
    got = nlf_defaults.digests(model)
    assert got == recorded, {k: (got.get(k), v) for k, v in recorded.items() if got.get(k) != v}
