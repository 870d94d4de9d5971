"""Stream order made deterministic: LiveStream, ClipPipeline and the model's own entry points with a bounded delay (tests/stream_hold.py:
a "hold") on one chosen HIP stream at a time.  At the sizes the suite runs, every kernel finishes long before the host enqueues the next
one, so any order of the streams gives the right bytes; behind a hold a consumer that is not ordered after its producer reads old bytes,
and the byte comparison fails.  For every hand-over the held run is then repeated with that one wait removed, and must fail.

Expected bytes never come from a pipeline: they are ``*_to_input -> clip_forward(cuts=) -> blend_output -> output_to_*`` by hand on the
default stream (test_gpu_finish._by_hand), computed once per configuration and shared.

Every held run first asserts, on the pipeline's own stream objects, that producer and consumer can run side by side at all
(stream_hold.overlaps): two streams that share a hardware queue run in order whatever the code does.

What the probes measured is printed as ``stream-order: ...`` lines (pytest -s); profiles/stream_order.txt keeps a record."""
import contextlib
import types

import numpy as np
import pytest
import torch

import finish_model as F
import stream_hold as SH
import test_gpu_cuts as TC
import test_gpu_finish as TF
import test_gpu_rgb as TR
from helpers import bsvd_keys
from seeded import seeded_state
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIGMA = TR.SIGMA
H, W = 16, 24
PAIRS = [("up", "comp"), ("comp", "down"), ("up", "down")]
MODES = {"up": [("up", 1)], "comp": [("comp", 1)], "down": [("down", 1)], "all": [("up", 1), ("comp", 2), ("down", 3)]}
LONGEST = 25                               # frames of the longest stream: latency + depth + 3 at depth 3 with the lagged schedule
SHORT = 6                                  # the second stream on the same object: shorter than the latency, everything comes out of flush()

# pix_fmt, picture, the pipelines' options, by-hand arguments (cuts / strength / dither / sigma / pad), feed(cut=True) at
CONFIGS = {
    "A1": ("rgb24", (H, W), dict(sigma=SIGMA, depth=1, overlap_blocks=False), dict(), None),
    "A2": ("rgb24", (H, W), dict(sigma=SIGMA, depth=2), dict(), None),
    "A3": ("rgb24", (H, W), dict(sigma=SIGMA, depth=3), dict(), None),
    "B": ("bgra", (H, W), dict(sigma=SIGMA, depth=2, strength=(0.4, 1.0), dither="random", dither_seed=F.SEED),
          dict(strength=(0.4, 1.0), dither="random"), 19),
    "C2": ("yuv420p", SH.C_SIZE, dict(sigma="auto", cuts="auto", strength=0.5, dither="ordered", depth=2, pad="reflect", frame_shape=SH.C_SIZE),
           dict(cuts="auto", strength=0.5, dither="ordered", seed=0, sigma="auto", pad="reflect", size=SH.C_SIZE), None),
    "C1": ("yuv420p", SH.C_SIZE, dict(sigma="auto", cuts="auto", strength=0.5, dither="ordered", depth=1, overlap_blocks=False, pad="reflect",
                                      frame_shape=SH.C_SIZE),
           dict(cuts="auto", strength=0.5, dither="ordered", seed=0, sigma="auto", pad="reflect", size=SH.C_SIZE), None),
    "D": ("rgba64le", (H, W), dict(sigma="auto", depth=2), dict(sigma="auto"), None),
}
ALL = dict(CONFIGS)
ALL["Bclip"] = CONFIGS["B"][:4] + (None,)          # ClipPipeline: the clips carry no feed(cut=True)


# ---- frames and the by-hand results ----------------------------------------------------------------------------------------------------------
_FRAMES, _WANT = {}, {}


def _frames(key, n):
    """n host frames of configuration ``key``: every frame different, the whole code range in use; shared, never written"""
    fmt = ALL[key][0]
    assert n <= LONGEST
    if fmt not in _FRAMES:
        n_, n = n, LONGEST                   # one clip per format: a shorter one is its beginning
        rs = np.random.RandomState(len(fmt))
        if fmt == "rgb24":
            a = rs.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
        elif fmt == "bgra":
            a = TF._frames("bgra", n, H, W, seed=91)
        elif fmt == "rgba64le":
            # a flat colour per frame under noise of a level of its own (3 ... 47 / 255): every frame has another estimate; both ends of
            # the code range in every frame; alpha over the whole range
            lvl = (3.0 + 2.0 * np.arange(n)) * 257.0
            a = rs.uniform(0.2, 0.8, (n, 1, 1, 4)) * 65535.0 + rs.standard_normal((n, H, W, 4)) * lvl[:, None, None, None]
            a = np.clip(np.rint(a), 0, 65535)
            a[:, 0, 0, :3], a[:, 0, 1, :3] = 0, 65535
            a[..., 3] = rs.randint(0, 65536, (n, H, W))
            a = a.astype(np.uint16)
        else:
            x, _ = SH.two_scene_clip()
            a = TC._margin_frames("yuv420p", x)                 # 23 frames: depth 2 with the lagged schedule
        a.setflags(write=False)
        _FRAMES[fmt] = a
        n = n_
    assert n <= len(_FRAMES[fmt])
    return _FRAMES[fmt][:n]


def _want(m, key, n, frame0=0, first=0):
    """the by-hand result of frames [first, first + n) of configuration ``key`` as a stream of its own whose dither index starts at
    ``frame0`` -> (bytes, sigma per frame, scene starts)"""
    fmt, _, _, hand, cut = ALL[key]
    k = (fmt, tuple(sorted((a, repr(b)) for a, b in hand.items())), n, frame0, first, cut)
    if k not in _WANT:
        fr = _frames(key, max(n + first, _len(key)))[first:first + n]
        kw = dict(cuts=[cut] if cut is not None and cut < n else None, strength=None, dither=None)
        kw.update(hand)
        info = {}
        got = TF._by_hand(m, fr, fmt, kw.pop("cuts"), kw.pop("strength"), kw.pop("dither"), frame0=frame0, info=info, **kw)
        got.setflags(write=False)
        _WANT[k] = (got, info["sigma"], info["cuts"])
    return _WANT[k]


def _len(key):
    """latency + depth + 3 at the configuration's depth: both rings turn once"""
    kw = ALL[key][2]
    depth = kw["depth"]
    overlap = kw.get("overlap_blocks", depth >= 2)
    return 16 + depth - 1 + (1 if overlap else 0) + depth + 3


# ---- holds -----------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _held(obj, method, holds, ms, after=None):
    """before every ``obj.method(...)`` one hold of ``mult * ms`` on each of ``holds`` = [(stream attribute, mult)]; ``after()`` behind it"""
    inner = getattr(obj, method)

    def call(*a, **k):
        for name, mult in holds:
            SH.hold(getattr(obj, name), mult * ms)
        r = inner(*a, **k)
        if after is not None:
            after()
        return r

    setattr(obj, method, call)
    try:
        yield
    finally:
        delattr(obj, method)


def _ms(ms, key=None):
    """the hold of configuration ``key``'s shape (None: 16 x 24) out of the ``hold_ms`` fixture's table"""
    return ms[ALL[key][1] if key else (H, W)]


def _live(m, key, what):
    from bsvd_amd.pipeline import LiveStream
    fmt, _, kw, _, _ = CONFIGS[key]
    live, _ = SH.on_distinct_queues(lambda: LiveStream(m, pix_fmt=fmt, **kw), PAIRS, "LiveStream %s (%s)" % (key, what))
    return live


def _run_live(live, key, frames, holds, ms, after=None, mutate=None, steady=False):
    """one stream through ``live`` with a hold before every step, flush() included -> (frames, last_sigma after each feed, last_cut after
    each feed).  ``mutate(live)``: a context manager entered behind the first feed (the slots exist then).  ``steady``: between any two
    feeds past the first ring period, torch.cuda.memory_allocated() is one value."""
    cut = CONFIGS[key][4]
    ms = _ms(ms, key)
    got, sig, cuts, mem = [], [], [], []
    with contextlib.ExitStack() as stack:
        stack.enter_context(_held(live, "_step", holds, ms, after))
        for k, fr in enumerate(frames):
            r = live.feed(fr, cut=True) if k == cut else live.feed(fr)
            if k == 0 and steady:
                assert len(frames) == live.latency + live.depth + 3 and live.latency_final
            if k == 0 and mutate is not None:
                stack.enter_context(mutate(live))
            if r is not None:
                got.append(r)
            sig.append(live.last_sigma)
            cuts.append(bool(live.last_cut))
            if k >= live.latency + live.depth:
                mem.append(torch.cuda.memory_allocated())
        got += live.flush()
    if steady and mem:
        assert len(set(mem)) == 1, ("device memory moved between feeds", mem)
    return np.stack(got), sig, cuts


def _check_live(m, live, key, got, n, mode, fresh=True):
    frames, sig, cuts = got
    want, want_sig, want_cuts = _want(m, key, n)
    assert frames.shape == want.shape and frames.dtype == want.dtype
    bad = [t for t in range(n) if not np.array_equal(frames[t], want[t])]
    assert not bad, "%s, hold on %s: frames %s differ from the by-hand bytes" % (key, mode, bad)
    if want.ndim == 4 and want.shape[-1] == 4:
        assert np.array_equal(frames[..., 3], _frames(key, n)[..., 3]), "alpha left its frame"
    lag = live.depth - 1
    if CONFIGS[key][2]["sigma"] == "auto":             # the estimate of the frame fed depth - 1 calls ago; None before, on a new object
        assert sig[lag:] == want_sig[:n - lag] and (not fresh or sig[:lag] == [None] * lag), (key, mode, sig, want_sig)
    else:
        assert sig == [None] * n
    if CONFIGS[key][2].get("cuts") == "auto":
        assert cuts == [t in want_cuts for t in range(n)], (key, mode, cuts, want_cuts)


STEP_LIMIT_MS = 5.0        # a step of these shapes is 0.4 ms (16 x 24) and 1.2 - 1.4 ms (30 x 42, estimator and detector): far beyond that, the
#                            measurement is not one of the device's work, and a hold of 10 x it would make every test here take minutes


@pytest.fixture(scope="module")
def hold_ms(model):     # noqa: F811
    """the hold's length per test shape: 3 ms, or 10 x the device time of one unheld LiveStream step where that is longer.  The step is
    timed by device events on the pipeline's own streams, from the end of a 2 ms hold on the upload stream (the host enqueues the step
    meanwhile) to the end of the download, in the steady state -- every launch plan of the ring period seen twice and captured, so the step
    is one graph replay.  Whatever the host adds inside the window (it did, in the middle of the suite: see profiles/stream_order.txt) only
    lengthens a reading: the shortest of six is the step."""
    import time
    from bsvd_amd.stream_plan import RING_PERIOD
    SH.calibrate(DEV)
    ms = {}
    for key in ("A2", "C2"):
        live = _live(model, key, "step time")
        frames = _frames(key, _len(key))
        warm = live.latency + 2 * RING_PERIOD + 2            # fill, first sightings (batched launches), second (captures)
        times, host = [], []
        for k in range(warm + 6):
            fr = frames[k % 6] if key == "C2" else frames[k % len(frames)]       # C: one scene
            if k >= warm:
                caps = model._stream_eng.stats["graph_captures"]
                SH.hold(live.up, 2.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(live.up)
                t0 = time.perf_counter()
                live.feed(fr)
                host.append(1e3 * (time.perf_counter() - t0))
                e1.record(live.down)
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                assert model._stream_eng.stats["graph_captures"] == caps, "the timed steps are replays"
            else:
                live.feed(fr)
        live.flush()
        SH.note("unheld LiveStream step %s (%s %d x %d): %s ms on the device (host time inside feed(): %s ms)"
                % ((key, CONFIGS[key][0]) + CONFIGS[key][1] + (", ".join("%.3f" % t for t in times), ", ".join("%.2f" % t for t in host))))
        step = min(times)
        assert step < STEP_LIMIT_MS, "an unheld step of %s took %.1f ms on the device, %.0f x what it takes alone" % (key, step, step / 0.4)
        ms[CONFIGS[key][1]] = max(SH.HOLD_MS, 10.0 * step)
        SH.note("hold used at %d x %d: %.2f ms (3 ms, or 10 x the step where that is longer)" % (CONFIGS[key][1] + (ms[CONFIGS[key][1]],)))
    return ms


# ---- item 2: the host pipelines under holds -------------------------------------------------------------------------------------------------
def test_stream_pairs_of_both_pipelines_can_run_side_by_side(model):     # noqa: F811
    """what every held test rests on, on its own: the three streams of a LiveStream and of a ClipPipeline as they come, pair by pair (noted,
    not asserted: streams share hardware queues), and after the rebuilds of stream_hold.on_distinct_queues (asserted there)"""
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    for cls in (LiveStream, ClipPipeline):
        obj = cls(model, sigma=SIGMA, depth=2)
        SH.note("%s as constructed: %s" % (cls.__name__, ", ".join("%s/%s %s" % (p, c, "overlap" if SH.overlaps(getattr(obj, p), getattr(obj, c))
                                                                                          else "share a queue") for p, c in PAIRS)))
        SH.SPARE.extend((obj.up, obj.comp, obj.down))
        obj, n = SH.on_distinct_queues(lambda: cls(model, sigma=SIGMA, depth=2), PAIRS, cls.__name__)
        assert all(SH.overlaps(getattr(obj, p), getattr(obj, c)) for p, c in PAIRS)
        assert not SH.overlaps(obj.comp, obj.comp)                   # the probe can say no: a stream does not overlap itself
        SH.note("%s: every pair overlaps after %d rebuild(s)" % (cls.__name__, n))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_live_stream_under_holds(model, hold_ms, key, mode):     # noqa: F811
    """a hold before every step on the upload, the compute or the download stream, or on all three with lengths 1 : 2 : 3: every frame, every
    alpha plane, last_sigma and last_cut are the by-hand result; then flush() and a second, short stream on the same object, held the same
    way; device memory does not move between feeds"""
    n = _len(key)
    live = _live(model, key, mode)
    got = _run_live(live, key, _frames(key, n), MODES[mode], hold_ms, steady=True)
    _check_live(model, live, key, got, n, mode)
    again = _run_live(live, key, _frames(key, n)[:SHORT], MODES[mode], hold_ms)
    _check_live(model, live, key, again, SHORT, mode + ", second stream", fresh=False)


def _clips(key, shift=0):
    """three clips of 3, 4 and 3 frames as (first frame, length); C: the first two hold the cut.  ``shift``: other frames of the same clip
    (the mutants': whatever an earlier run left in a reused block is then not what the mutant should have read)"""
    if key == "C2":
        s = SH.C_LENGTHS[0]
        return [(s - 2, 3), (s - 2, 4), (0, 3)]
    return [(shift, 3), (shift + 3, 4), (shift + 7, 3)]


def _pipe(m, key, what):
    from bsvd_amd.pipeline import ClipPipeline
    fmt, _, kw, _, _ = CONFIGS[key]
    pipe, _ = SH.on_distinct_queues(lambda: ClipPipeline(m, pix_fmt=fmt, **kw), PAIRS, "ClipPipeline %s (%s)" % (key, what))
    return pipe


def _clip_wants(m, key, frame0=0, shift=0):
    out = []
    for first, n in _clips(key, shift):
        out.append(_want(m, key.replace("B", "Bclip"), n, frame0=frame0, first=first))
        frame0 += n
    return out


def _run_clips(pipe, key, holds, ms, api, after=None, shift=0):
    """-> ([result per clip], [last_cuts behind each submit])"""
    fr = _frames(key, _len(key))
    clips = [fr[a:a + n] for a, n in _clips(key, shift)]
    cuts = []
    with _held(pipe, "submit", holds, _ms(ms, key), lambda: (cuts.append(pipe.last_cuts), after and after())):
        if api == "run":
            return list(pipe.run(iter(clips))), cuts
        for c in clips:                                     # depth 2, three clips: the third submit finds the ring full
            pipe.submit(c)
        return list(pipe.results()), cuts


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("key", ["B", "C2"])
def test_clip_pipeline_under_holds(model, hold_ms, key, mode):     # noqa: F811
    """three clips of alternating length at depth 2 through run(), then through submit() / results() with the ring full, a hold before
    every submit: the by-hand bytes with the pipeline's running dither index, and every clip's cuts"""
    pipe = _pipe(model, key, mode)
    frame0 = 0
    for api in ("run", "submit"):
        got, cuts = _run_clips(pipe, key, MODES[mode], hold_ms, api)
        wants = _clip_wants(model, key, frame0)
        assert len(got) == len(wants) == 3
        for i, (g, (w, _, wc)) in enumerate(zip(got, wants)):
            assert g.dtype == w.dtype and np.array_equal(g, w), "%s, hold on %s, %s: clip %d differs from the by-hand bytes" % (key, mode, api, i)
        if CONFIGS[key][2].get("cuts") == "auto":
            assert cuts == [wc for _, _, wc in wants] and cuts[0] == [2] and cuts[2] == []
        frame0 += sum(n for _, n in _clips(key))


def test_record_stream_holds_under_an_allocation_burst(model, hold_ms):     # noqa: F811
    """``x.record_stream(self.comp)`` is not mutated (what its absence does depends on when the allocator hands the block out again); it is
    held to its purpose from the other side: the compute stream held, and after every step a burst of allocations of x's size on the upload
    stream, each filled with NaN there.  A block of x handed out before the compute stream has read it would carry NaN into the frames."""
    key = "C2"
    n = _len(key)
    live = _live(model, key, "allocation burst")
    hp, wp = 32, 44

    def burst():
        with torch.cuda.stream(live.up):
            for t in [torch.empty((1, 4, hp, wp), dtype=torch.float32, device=DEV) for _ in range(8)]:
                t.fill_(float("nan"))

    got = _run_live(live, key, _frames(key, n), MODES["comp"], hold_ms, after=burst, steady=True)
    assert live.geom.net_h == hp and live.geom.net_w == wp
    _check_live(model, live, key, got, n, "comp + burst")


# ---- item 3: the model's entry points on the caller's stream ---------------------------------------------------------------------------------
CUT = 21
_FP32 = {}


def _net(model, precision):     # noqa: F811
    if precision == "f16x3":
        return model
    if "m" not in _FP32:
        import bsvd_amd
        st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32), 11)
        m = bsvd_amd.BSVD(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32, pretrain_ckpt=None,
                          precision="fp32")
        m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
        _FP32["m"] = m.to(DEV)
    return _FP32["m"]


_ENTRY = {}


def _entry_case(m, precision):
    """(x [T,4,16,24] on the device, clip_forward(x, cuts=[CUT]) run plainly), T = 2 ring periods + shift_num + 2: first sightings (batched
    launches), second (capture and replay) and later ones (replay)"""
    if precision not in _ENTRY:
        from bsvd_amd.stream_plan import RING_PERIOD
        T = 2 * RING_PERIOD + m.shift_num + 2
        rs = np.random.RandomState(7)
        x = rs.uniform(0.0, 1.0, (T, 4, H, W)).astype(np.float32)
        x[:, 3] = SIGMA
        x = torch.from_numpy(x).to(DEV)
        want = m.clip_forward(x, cuts=[CUT])
        torch.cuda.synchronize()
        _ENTRY[precision] = (x, want)
    return _ENTRY[precision]


def _streams(what):
    """a caller's stream s, another stream o and the default stream d, s able to run beside both"""
    ns, _ = SH.on_distinct_queues(lambda: types.SimpleNamespace(s=torch.cuda.Stream(DEV), o=torch.cuda.Stream(DEV), d=torch.cuda.default_stream(DEV)),
                                  [("s", "o"), ("s", "d")], what)
    return ns


def _per_frame(m, api, x, s, ms, call_on=None):
    """under stream s: the reused input buffer filled with NaN, a hold, frame k copied in, the entry point called (under ``call_on``: the
    mutant), the result cloned there; one synchronise at the end.  Whatever runs on another stream than s runs before the copy."""
    buf = torch.empty_like(x[:1])
    ms = _ms(ms)
    torch.cuda.synchronize()
    feed = getattr(m, api)
    tail = m.shift_num + (1 if api == "feed_overlapped" else 0)
    outs = []
    m.reset()
    try:
        with torch.cuda.stream(s):
            for k in range(x.shape[0] + tail):
                if k < x.shape[0]:
                    buf.fill_(float("nan"))
                SH.hold(s, ms)
                if k < x.shape[0]:
                    buf.copy_(x[k:k + 1])
                with torch.cuda.stream(call_on or s):
                    y = feed(buf, cut=(k == CUT)) if k < x.shape[0] else feed(None)
                    if y is not None:
                        outs.append(y.clone())
            with torch.cuda.stream(call_on or s):
                assert (m.feed_overlapped(None, last=True) if api == "feed_overlapped" else m.feedin_one_element(None)) is None
        torch.cuda.synchronize()
    finally:
        m.reset()
    return torch.cat(outs)


def _whole_clip(m, fn, x, s, ms, calls, call_on=None):
    buf = torch.empty_like(x)
    ms = _ms(ms)
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for _ in range(calls):
            buf.fill_(float("nan"))
            SH.hold(s, ms)
            buf.copy_(x)
            with torch.cuda.stream(call_on or s):
                outs.append(fn(buf).clone())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("api", ["feedin_one_element", "feed_overlapped"])
def test_per_frame_entry_points_run_on_the_callers_stream(model, hold_ms, api, precision):     # noqa: F811
    m = _net(model, precision)
    x, want = _entry_case(m, precision)
    ns = _streams(api)
    got = _per_frame(m, api, x, ns.s, hold_ms)
    assert not torch.isnan(got).any() and torch.equal(got, want)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("chunk,overlap", [(1, True), (1, False), (2, True), (2, False)])
def test_clip_entry_points_run_on_the_callers_stream(model, hold_ms, chunk, overlap, precision):     # noqa: F811
    """streaming_forward three times (batched launches, capture, replay) and clip_forward, each behind a hold and a NaN-filled buffer"""
    m = _net(model, precision)
    x, want = _entry_case(m, precision)
    ns = _streams("streaming_forward")
    keep = m.stream_chunk, m.stream_overlap
    try:
        m.stream_chunk, m.stream_overlap = chunk, overlap
        for y in _whole_clip(m, lambda b: m.streaming_forward(b, cuts=[CUT]), x, ns.s, hold_ms, 3):
            assert torch.equal(y, want)
        assert m._stream_engs[chunk].stats["graph_replays"] > 0
    finally:
        m.stream_chunk, m.stream_overlap = keep
    if chunk == 1 and overlap:
        (y,) = _whole_clip(m, lambda b: m.clip_forward(b, cuts=[CUT]), x, ns.s, hold_ms, 1)
        assert torch.equal(y, want)


# ---- item 4: one mutant per hand-over ---------------------------------------------------------------------------------------------------------
# Each runs only after the unmutated held run has passed in the same test, on an object of its own that is thrown away, and is followed by a
# device synchronise.  A mutant reads old bytes of buffers that stay allocated: the slots' buffers, the rings, pinned memory -- and the
# per-step device results, which the test keeps alive (``keep``) so that no block goes back to the allocator while a held stream still
# has a copy of it to make.
def _keeper(obj, keep):
    def after():
        for s in obj.slots or ():
            keep.extend(t for t in (s.dev_out, s.dev_alpha, s.dev_in) if t is not None)
    return after


def _mutant_live(m, key, mode, ms, mutate):
    """the unmutated held run passes; the same run with ``mutate`` fails -> (got, want) of the mutated run"""
    n = _len(key)
    live = _live(m, key, "before the mutant")
    _check_live(m, live, key, _run_live(live, key, _frames(key, n), MODES[mode], ms), n, mode)
    live = _live(m, key, "mutant")
    keep = []
    try:
        got = _run_live(live, key, _frames(key, n), MODES[mode], ms, after=_keeper(live, keep), mutate=mutate)
    finally:
        torch.cuda.synchronize()
        m.reset()
    return got, _want(m, key, n)


def _differ(got, want):
    return [t for t in range(len(want)) if not np.array_equal(got[t], want[t])]


def _all_slots(name, method):
    """the mutant: ``method`` of event ``name`` of every slot is a no-op"""
    @contextlib.contextmanager
    def mutate(obj):
        with contextlib.ExitStack() as stack:
            for s in obj.slots:
                stack.enter_context(SH.without(getattr(s, name), method))
            yield
    return mutate


MUTANT_SHIFT = {"run": 10, "submit": 13}          # other frames than the run before, and than each other


def _mutant_clip(m, mode, ms, mutate):
    key = "B"
    pipe = _pipe(m, key, "before the mutant")
    for api, frame0 in (("run", 0), ("submit", 10)):
        got, _ = _run_clips(pipe, key, MODES[mode], ms, api)
        assert all(np.array_equal(g, w) for g, (w, _, _) in zip(got, _clip_wants(m, key, frame0)))
    out = []
    for api in ("run", "submit"):
        pipe = _pipe(m, key, "mutant")
        keep = []
        try:
            with mutate(pipe):
                got, _ = _run_clips(pipe, key, MODES[mode], ms, api, after=_keeper(pipe, keep), shift=MUTANT_SHIFT[api])
        finally:
            torch.cuda.synchronize()
        wants = _clip_wants(m, key, shift=MUTANT_SHIFT[api])
        out.append([i for i, (g, (w, _, _)) in enumerate(zip(got, wants)) if not np.array_equal(g, w)])
    return out


@pytest.mark.parametrize("which", ["live", "clip"])
def test_mutant_compute_does_not_wait_for_the_upload(model, hold_ms, which):     # noqa: F811
    """4a: ``comp.wait_event(slot.uploaded)`` removed, the upload stream held: the conversion reads the slot's device buffer before the copy"""
    mutate = lambda obj: SH.without(obj.comp, "wait_event")     # noqa: E731
    if which == "live":
        (frames, _, _), (want, _, _) = _mutant_live(model, "B", "up", hold_ms, mutate)
        bad = _differ(frames, want)
        SH.note("mutant 4a live: %d of %d frames differ" % (len(bad), len(want)))
        assert bad
    else:
        bad = _mutant_clip(model, "up", hold_ms, mutate)
        SH.note("mutant 4a clip: clips that differ, run() %s, submit() %s" % tuple(bad))
        assert bad[0] and bad[1]


@pytest.mark.parametrize("which", ["live", "clip"])
def test_mutant_download_does_not_wait_for_the_compute(model, hold_ms, which):     # noqa: F811
    """4b: ``down.wait_event(slot.computed)`` removed, the compute stream held: the download copies the result before it is computed"""
    mutate = lambda obj: SH.without(obj.down, "wait_event")     # noqa: E731
    if which == "live":
        (frames, _, _), (want, _, _) = _mutant_live(model, "B", "comp", hold_ms, mutate)
        bad = _differ(frames, want)
        SH.note("mutant 4b live: %d of %d frames differ" % (len(bad), len(want)))
        assert bad
    else:
        bad = _mutant_clip(model, "comp", hold_ms, mutate)
        SH.note("mutant 4b clip: clips that differ, run() %s, submit() %s" % tuple(bad))
        assert bad[0] and bad[1]


@pytest.mark.parametrize("which", ["live", "clip"])
def test_mutant_host_reads_before_the_download(model, hold_ms, which):     # noqa: F811
    """4c: ``slot.downloaded.synchronize()`` removed (LiveStream._pop, _Ticket.finish), the download stream held: the host copies the pinned
    buffer before the download has filled it"""
    mutate = _all_slots("downloaded", "synchronize")
    if which == "live":
        (frames, _, _), (want, _, _) = _mutant_live(model, "A2", "down", hold_ms, mutate)
        bad = _differ(frames, want)
        SH.note("mutant 4c live: %d of %d frames differ" % (len(bad), len(want)))
        assert bad
    else:
        bad = _mutant_clip(model, "down", hold_ms, mutate)
        SH.note("mutant 4c clip: clips that differ, run() %s, submit() %s" % tuple(bad))
        assert bad[0] and bad[1]


def test_mutant_host_decides_before_the_score(model, hold_ms):     # noqa: F811
    """4d: ``_scored.synchronize()`` removed, the upload stream held: the host reads the pinned sum before the 8-byte copy -- the previous
    frame's -- and decides the cut from it"""
    mutate = lambda live: SH.without(live._scored, "synchronize")     # noqa: E731
    (frames, _, cuts), (want, _, want_cuts) = _mutant_live(model, "C2", "up", hold_ms, mutate)
    bad = _differ(frames, want)
    found = [t for t, c in enumerate(cuts) if c]
    SH.note("mutant 4d: cuts found at %s (by hand: %s), %d of %d frames differ" % (found, want_cuts, len(bad), len(want)))
    assert found != want_cuts or bad


def test_mutant_host_reads_sigma_before_the_download(model, hold_ms):     # noqa: F811
    """4e: 4c seen from the sigma side: ``last_sigma`` is read from the slot's pinned 4 bytes before the download has written them"""
    (_, sig, _), (_, want_sig, _) = _mutant_live(model, "D", "down", hold_ms, _all_slots("downloaded", "synchronize"))
    n = len(want_sig)
    bad = [t for t in range(n - 1) if sig[t + 1] != want_sig[t]]
    SH.note("mutant 4e: %d of %d values of last_sigma differ" % (len(bad), n - 1))
    assert len(set(want_sig)) > n // 2 and bad


@pytest.mark.parametrize("api", ["feedin_one_element", "streaming_forward"])
def test_mutant_entry_point_called_under_another_stream(model, hold_ms, api):     # noqa: F811
    """4f: the entry point called under another stream than the one that wrote x -- what a launch on a wrong stream inside the engine would
    be: it runs before the copy, reads the NaN (or the frame before) and shows"""
    x, want = _entry_case(model, "f16x3")
    ns = _streams("mutant 4f")
    if api == "feedin_one_element":
        assert torch.equal(_per_frame(model, api, x, ns.s, hold_ms), want)
        got = _per_frame(model, api, x, ns.s, hold_ms, call_on=ns.o)
    else:
        fn = lambda b: model.streaming_forward(b, cuts=[CUT])     # noqa: E731
        assert torch.equal(_whole_clip(model, fn, x, ns.s, hold_ms, 1)[0], want)
        got = _whole_clip(model, fn, x, ns.s, hold_ms, 1, call_on=ns.o)[0]
    bad = [t for t in range(want.shape[0]) if not torch.equal(got[t], want[t])]
    SH.note("mutant 4f %s: %d of %d frames differ" % (api, len(bad), want.shape[0]))
    assert bad


def test_without_works_on_streams_events_and_tensors():
    s, e, t = torch.cuda.Stream(DEV), torch.cuda.Event(), torch.zeros(4, device=DEV)
    for obj, method in ((s, "wait_event"), (e, "synchronize"), (t, "record_stream")):
        with SH.without(obj, method):
            assert getattr(obj, method)(*(() if method == "synchronize" else (e if method == "wait_event" else s,))) is None
            assert method in obj.__dict__
        assert method not in obj.__dict__
    e.record(s)
    s.wait_event(e)
    e.synchronize()
    t.record_stream(s)
