"""Scene cuts on the MI355X: the schedules with the scene starts given, the steady state after a cut, the detector's two kernels against
tests/scene_model.py, and LiveStream / ClipPipeline with cuts='auto'.

The contract (tests/test_cuts_cpu.py holds the host logic to it on the CPU): every frame is, bit for bit, what ``clip_forward`` gives for
its scene run alone.  The clip: 40 frames of 32 x 48 in scenes of 5, 1, 2, 19 and 13 frames that differ by O(1)."""
import numpy as np
import pytest
import torch

import scene_model as M
from helpers import bsvd_keys
from seeded import seeded_state, seeded_clip

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C32 = dict(chns=[32, 64, 128], mid_ch=32, interm_ch=32)
C64 = dict(chns=[64, 128, 256], mid_ch=64, interm_ch=64)
H, W = 32, 48
LENGTHS = (5, 1, 2, 19, 13)
STARTS = [int(v) for v in np.cumsum((0,) + LENGTHS[:-1])]          # 0, 5, 6, 8, 27
T = sum(LENGTHS)

_MODELS = {}


def _model(precision="f16x3", cfg="c32"):
    """one model per (arithmetic mode, network), shared by every case"""
    if (precision, cfg) not in _MODELS:
        import bsvd_amd
        c = C32 if cfg == "c32" else C64
        m = bsvd_amd.BSVD(norm="none", act="relu6", pretrain_ckpt=None, precision=precision, **c)
        st = seeded_state(bsvd_keys(c["chns"], c["mid_ch"], 4, 3, c["interm_ch"]), 13)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
        _MODELS[precision, cfg] = m.to(DEV).eval()
    return _MODELS[precision, cfg]


def _scenes(starts, n):
    edges = sorted(set(starts) | {0}) + [n]
    return list(zip(edges[:-1], edges[1:]))


_CLIPS = {}


def _clip(n=T, starts=STARTS, seed=6):
    key = (n, tuple(starts), seed)
    if key not in _CLIPS:
        x = torch.from_numpy(seeded_clip((1, n, 4, H, W), seed, kind="sigma30"))[0].clone()
        for k, (a, b) in enumerate(_scenes(starts, n)):
            x[a:b, :3] += float(k)
        _CLIPS[key] = x.to(DEV)
    return _CLIPS[key]


_WANT = {}


def _want(precision, cfg="c32", n=T, starts=STARTS, seed=6):
    """the reference: each scene through clip_forward, alone.  Computed once per mode, shared, never written to"""
    key = (precision, cfg, n, tuple(starts), seed)
    if key not in _WANT:
        m, x = _model(precision, cfg), _clip(n, starts, seed)
        _WANT[key] = torch.cat([m.clip_forward(x[a:b]) for a, b in _scenes(starts, n)])
    return _WANT[key]


def _per_frame(m, x, starts, api):
    outs = []
    try:
        if api == "feedin_one_element":
            for t in range(x.shape[0]):
                outs.append(m.feedin_one_element(x[t:t + 1], cut=t in starts))
            for _ in range(m.shift_num):
                outs.append(m.feedin_one_element(None))
            assert m.feedin_one_element(None) is None
            lat = m.shift_num
        else:
            for t in range(x.shape[0]):
                outs.append(m.feed_overlapped(x[t:t + 1], cut=t in starts))
            for _ in range(m.shift_num + 1):
                outs.append(m.feed_overlapped(None))
            assert m.feed_overlapped(None, last=True) is None
            lat = m.shift_num + 1
    finally:
        m.reset()
    assert all(o is None for o in outs[:lat]) and all(o is not None for o in outs[lat:])       # no step emits None because of a cut
    return torch.cat(outs[lat:])


# ------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_the_clip_can_tell(precision):
    """run as one scene, the frames on both sides of every cut differ from the per-scene result by far more than rounding"""
    m, want = _model(precision), _want(precision)
    whole = m.clip_forward(_clip())
    for s in STARTS[1:]:
        assert float((whole[s] - want[s]).abs().max()) > 1e-2 and float((whole[s - 1] - want[s - 1]).abs().max()) > 1e-2


@pytest.mark.parametrize("precision,api", [("f16x3", "feedin_one_element"), ("fp32", "feedin_one_element"), ("f16", "feedin_one_element"),
                                           ("f16x3", "feed_overlapped"), ("fp32", "feed_overlapped")])
def test_per_frame_feeds_with_cut_flags(precision, api):
    m = _model(precision)
    got = _per_frame(m, _clip(), set(STARTS[1:]), api)
    assert torch.equal(got, _want(precision))
    assert not m._stream_eng.cuts.pending


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_streaming_forward_with_cuts(precision, chunk, overlap):
    """chunk 2: no chunk spans a cut, so the scenes of 5, 1, 19 and 13 frames end in a one-frame chunk in mid-stream"""
    m = _model(precision)
    keep = m.stream_chunk, m.stream_overlap
    try:
        m.stream_chunk, m.stream_overlap = chunk, overlap
        got = m.streaming_forward(_clip(), cuts=STARTS)
        assert m._stream_engs[chunk].chunk == chunk
        assert torch.equal(got, _want(precision))
        assert torch.equal(m.streaming_forward(list(_clip().split(1)), cuts=iter(STARTS[1:])), _want(precision))     # the same plans again
    finally:
        m.stream_chunk, m.stream_overlap = keep


@pytest.mark.parametrize("mode", ["clip", "stream"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_forward_with_cuts(precision, mode):
    m = _model(precision)
    keep = m.engine_mode
    try:
        m.engine_mode = mode
        x = _clip()
        got = m.forward(x[None, :, :3], noise_map=x[None, :, 3:], cuts=STARTS[1:])
        assert m.last_mode == mode and torch.equal(got[0], _want(precision))
        assert torch.equal(m.forward(x[None], cuts=[0])[0], m.forward(x[None])[0])             # 0 says nothing new
    finally:
        m.engine_mode = keep
    with pytest.raises(ValueError, match="outside"):
        m.forward(x[None], cuts=[T])


def test_c64_three_scenes():
    starts = [0, 7, 18]
    m, x = _model("f16x3", "c64"), _clip(24, starts, seed=9)
    got = _per_frame(m, x, set(starts[1:]), "feedin_one_element")
    assert torch.equal(got, _want("f16x3", "c64", 24, starts, seed=9))


def test_no_cut_is_what_it_was():
    """cut=False / cuts=None / cuts={0}: the plan table and the frames of a run without the argument"""
    m = _model("f16x3")
    x = _clip()[:30]
    m.release_stream_buffers()
    want = _per_frame(m, x, set(), "feedin_one_element")
    eng = m._stream_eng
    plans = len(eng.plans)
    outs = []
    for t in range(30):
        outs.append(m.feedin_one_element(x[t:t + 1]))
    for _ in range(m.shift_num + 1):
        outs.append(m.feedin_one_element(None))
    m.reset()
    assert torch.equal(torch.cat([o for o in outs if o is not None]), want) and len(eng.plans) == plans
    assert torch.equal(_per_frame(m, x, {0}, "feedin_one_element"), want) and len(eng.plans) == plans
    assert torch.equal(m.streaming_forward(x, cuts=[0]), m.streaming_forward(x))


# ------------------------------------------------------------------------------------------------ steady state after a cut
def _counts(eng):
    return dict(eng.stats, plans=len(eng.plans))


@pytest.mark.parametrize("api", ["feedin_one_element", "feed_overlapped"])
def test_steady_state_after_a_cut_and_recurring_cut_phases(api):
    from bsvd_amd.stream_plan import RING_PERIOD
    m = _model("f16x3")
    m.release_stream_buffers()                   # a table of its own: what was seen before is part of the statement
    x = _clip()
    feed = getattr(m, api)
    try:
        log = []
        for t in range(40 + 3 * RING_PERIOD):
            feed(x[t % T:t % T + 1], cut=t == 6)
            log.append(_counts(m._stream_eng))
        # the cut has left the pipeline: the stream is back on the graphs of its steady state, one replay per step
        a, b = log[-2 * RING_PERIOD - 1], log[-1]
        for name in ("graph_captures", "batch_launches", "plans"):
            assert a[name] == b[name], (name, a, b)
        assert b["graph_replays"] - a["graph_replays"] == 2 * RING_PERIOD
        m.reset()
        # a second stream: cuts at the same ring phase three times.  First sighting: batched launches; second: captures; third: replays only
        log = []
        cuts = (45, 45 + 3 * RING_PERIOD, 45 + 6 * RING_PERIOD)       # (another phase than the first stream's cut)
        n = cuts[2] + m.shift_num + 3
        for t in range(n):
            feed(x[t % T:t % T + 1], cut=t in cuts)
            log.append(_counts(m._stream_eng))
        first, second, third = [(log[c - 1], log[c + m.shift_num + 2]) for c in cuts]
        assert first[1]["batch_launches"] > first[0]["batch_launches"] and first[1]["plans"] > first[0]["plans"]
        assert second[1]["graph_captures"] > second[0]["graph_captures"]
        assert second[1]["batch_launches"] == second[0]["batch_launches"] and second[1]["plans"] == second[0]["plans"]
        for name in ("graph_captures", "batch_launches", "plans"):
            assert third[1][name] == third[0][name], (name, third)
        assert third[1]["graph_replays"] - third[0]["graph_replays"] == m.shift_num + 3
    finally:
        m.reset()


# ------------------------------------------------------------------------------------------------ the detector against the model
def _field(Tn, C, Hp, Wp, seed):
    rs = np.random.default_rng(seed)
    x = rs.uniform(-0.2, 1.2, (Tn, C, Hp, Wp)).astype(np.float32)
    x[:, :, 1::7, 2::5] = (np.arange(x[:, :, 1::7, 2::5].size).reshape(x[:, :, 1::7, 2::5].shape) % 256 + 0.5) / 255.0      # halves: 0.5, 1.5, ... (rint: to even)
    x[0, 0, 3, 5], x[0, 1, 4, 6], x[0, 2, 17 % Hp, 33], x[-1, 1, 2, 40] = np.nan, np.inf, -np.inf, np.nan
    x[0, 2, 5, 7], x[0, 0, 6, 8] = -3.0, 9.0
    return x


DETECT = {"32x48": (1, 4, 32, 48, None), "32x48_T5": (5, 4, 32, 48, None), "36x52_in_34x50": (5, 4, 36, 52, (34, 50)), "8x48": (5, 4, 8, 48, None),
          "64x96": (5, 4, 64, 96, None), "64x96_3ch": (5, 3, 64, 96, None), "64x96_T1_3ch": (1, 3, 64, 96, None), "33x50_scalar_rows": (5, 3, 33, 50, None),
          "48x80_in_47x79": (2, 4, 48, 80, (47, 79))}


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("name", sorted(DETECT))
def test_grid_and_sad_equal_the_model_bit_for_bit(name, with_prev):
    from bsvd_amd.frame_io import scene_scores
    Tn, C, Hp, Wp, picture = DETECT[name]
    x = _field(Tn, C, Hp, Wp, len(name))
    if picture is not None:                                   # nothing outside the picture may count
        x[:, :, picture[0]:, :] = np.nan
        x[:, :, :, picture[1]:] = np.nan
    want_g = M.grid(x, picture)
    prev = None
    if with_prev:
        prev = np.random.default_rng(5).integers(0, 261121, want_g.shape[1:]).astype(np.int32)
    want_s = M.sad(want_g, prev)
    sad, grid = scene_scores(torch.from_numpy(x).to(DEV), picture=picture, prev=None if prev is None else torch.from_numpy(prev).to(DEV))
    assert grid.dtype == torch.int32 and tuple(grid.shape) == want_g.shape and sad.dtype == torch.int64 and tuple(sad.shape) == (Tn,)
    assert np.array_equal(grid.cpu().numpy().astype(np.int64), want_g)
    assert np.array_equal(sad.cpu().numpy(), want_s)
    if want_g.size:
        assert want_g.max() <= 261120 and want_g.min() >= 0 and (with_prev or want_s[0] == 0) and (Tn == 1 or want_s[1:].min() > 0)
    else:
        assert not sad.cpu().numpy().any()


def test_scene_cuts_is_the_models_decision():
    from bsvd_amd.frame_io import scene_cuts, scene_scores
    x, starts = M.margin_clip(64, 96, seed=0)
    xd = torch.from_numpy(x).to(DEV)
    assert scene_cuts(xd) == starts[1:] == M.cuts(x)[0]
    assert scene_cuts(xd, threshold=1000.0) == []
    # a stream fed frame by frame, the previous grid handed on: the same sums as the clip at once
    sad, grid = scene_scores(xd)
    prev, one = None, []
    for t in range(x.shape[0]):
        s, g = scene_scores(xd[t:t + 1], prev=prev)
        prev = g[0]
        one.append(int(s[0]))
    assert one == sad.tolist()


# ------------------------------------------------------------------------------------------------ the pipelines
def _margin_frames(pix_fmt, x):
    """the margin clip (grey: R = G = B) as the pipeline's host frames: RGB24 [T,H,W,3], or yuv420p with limited-range luma and neutral chroma"""
    u8 = np.rint(x[:, :3] * 255.0).astype(np.uint8)
    if pix_fmt == "rgb24":
        return np.ascontiguousarray(u8.transpose(0, 2, 3, 1))
    n, _, h, w = u8.shape
    y = np.rint(16.0 + 219.0 / 255.0 * u8[:, 0].astype(np.float64)).astype(np.uint8).reshape(n, -1)
    return np.concatenate([y, np.full((n, h * w // 2), 128, np.uint8)], axis=1)


def _to_input(pix_fmt, frames, Hh, Ww, sigma):
    from bsvd_amd import frame_io as F
    dev = torch.from_numpy(frames).to(DEV)
    return F.frames_to_input(dev, sigma) if pix_fmt == "rgb24" else F.yuv_to_input(dev, Hh, Ww, pix_fmt, sigma=sigma)


def _stream(live, frames, flags=None):
    got, found, scores = [], [], []
    for i, fr in enumerate(frames):
        r = live.feed(fr) if flags is None else live.feed(fr, cut=flags[i])
        if r is not None:
            got.append(r)
        if live.last_cut:
            found.append(i)
        scores.append(live.last_cut_score)
    got += live.flush()
    return np.stack(got), found, scores


@pytest.mark.parametrize("pix_fmt,depth,overlap", [("rgb24", 1, False), ("rgb24", 2, True), ("rgb24", 2, False), ("yuv420p", 2, True), ("yuv420p", 1, False)])
def test_live_stream_auto(pix_fmt, depth, overlap):
    from bsvd_amd.pipeline import LiveStream
    m = _model("f16x3")
    Hh, Ww = 64, 96
    x, starts = M.margin_clip(Hh, Ww, seed=0)
    frames = _margin_frames(pix_fmt, x)
    # the conditions of the margin, on the tensor the device converts the frames to (the model alone decides this)
    xin = _to_input(pix_fmt, frames, Hh, Ww, 0.1).cpu().numpy()
    want_cuts, want_scores = M.cuts(xin)
    assert want_cuts == starts[1:]
    assert all(s >= 20.0 if t in starts[1:] else s <= 5.0 for t, s in enumerate(want_scores))
    kw = dict(sigma=0.1, depth=depth, overlap_blocks=overlap, pix_fmt=pix_fmt, frame_shape=(Hh, Ww))
    live = LiveStream(m, cuts="auto", **kw)
    assert live.last_cut_score is None and not live.last_cut
    got, found, scores = _stream(live, frames)
    assert found == starts[1:]
    assert scores == [float(s) for s in want_scores]
    ref = LiveStream(m, **kw)
    assert ref.latency == live.latency
    want, none_found, _ = _stream(ref, frames, [t in starts[1:] for t in range(len(frames))])
    assert none_found == [] and got.dtype == want.dtype and got.shape == frames.shape and np.array_equal(got, want)
    plain, _, _ = _stream(LiveStream(m, **kw), frames)
    assert not np.array_equal(plain, want)                    # the flags did something
    # a second stream through the same object starts from nothing: frame 0 scores 0 again
    again, found2, scores2 = _stream(live, frames[:6])
    assert scores2 == scores[:6] and found2 == [t for t in starts[1:] if t < 6]
    with pytest.raises(ValueError, match="finds the cuts itself"):
        live.feed(frames[0], cut=True)


def test_live_stream_auto_static_scene_has_no_cut():
    from bsvd_amd.pipeline import LiveStream
    m = _model("f16x3")
    x, _ = M.margin_clip(64, 96, lengths=(40,), seed=3)
    frames = _margin_frames("rgb24", x)
    live = LiveStream(m, sigma=0.1, depth=2, cuts="auto", frame_shape=(64, 96))
    got, found, scores = _stream(live, frames)
    assert found == [] and max(scores) < 5.0 and scores[0] == 0.0 and min(scores[1:]) > 0.0
    want, _, _ = _stream(LiveStream(m, sigma=0.1, depth=2, frame_shape=(64, 96)), frames)
    assert np.array_equal(got, want)


def test_live_stream_auto_with_pad_scores_the_picture():
    from bsvd_amd import frame_io as F
    from bsvd_amd.pipeline import LiveStream
    m = _model("f16x3")
    x, starts = M.margin_clip(64, 96, lengths=(4, 4), seed=2)
    frames = _margin_frames("rgb24", x)[:, :50, :70]          # 50 x 70 inside 52 x 72: GH, GW = 3, 4
    frames = np.ascontiguousarray(frames)
    xin = F.frames_to_input(torch.from_numpy(frames).to(DEV), 0.1, pad_to=F.network_size(50, 70)).cpu().numpy()
    want = [float(s) for s in M.cuts(xin, picture=(50, 70))[1]]
    live = LiveStream(m, sigma=0.1, depth=2, cuts="auto", pad="reflect", frame_shape=(50, 70))
    got, found, scores = _stream(live, frames)
    assert scores == want and found == starts[1:] and got.shape == frames.shape


@pytest.mark.parametrize("mode", ["clip", "stream"])
def test_clip_pipeline_auto(mode):
    from bsvd_amd import frame_io as F
    from bsvd_amd.pipeline import ClipPipeline
    m = _model("f16x3")
    x, starts = M.margin_clip(64, 96, seed=0)
    frames = _margin_frames("rgb24", x)
    keep = m.engine_mode
    try:
        m.engine_mode = mode
        pipe = ClipPipeline(m, sigma=0.1, cuts="auto")
        got = list(pipe.run([frames, frames[:9]]))
        assert pipe.last_cuts == [t for t in starts[1:] if t < 9]
        xin = F.frames_to_input(torch.from_numpy(frames).to(DEV), 0.1)
        want = F.output_to_frames(m.clip_forward(xin, cuts=starts)).cpu().numpy()
        assert np.array_equal(got[0], want) and np.array_equal(got[1], F.output_to_frames(m.clip_forward(xin[:9], cuts=[4])).cpu().numpy())
        assert not np.array_equal(got[0], list(ClipPipeline(m, sigma=0.1).run([frames]))[0])
    finally:
        m.engine_mode = keep
