"""The pipeline option matrix on the device: every row of tests/pipeline_matrix.py through LiveStream / ClipPipeline, byte for byte against
the synchronous composition of tests/pipeline_by_hand.py (no pipeline object on that side), which in turn is held to the numpy models on
every row, stream and clip.  Per feed: ``latency``, the number of None returns, ``last_sigma`` /
``last_noise_curve`` (the bits of the estimate of the frame fed ``depth - 1`` calls ago), ``last_cut_score`` / ``last_cut`` (the scores of
this stream alone), alpha with its frame.  Stream shapes: A one stream past a turn of the rings; B six frames, flush(), a second stream;
C a stream, flush(), another frame size on the same object.  Then the mutants: one value fault at a time patched into bsvd_amd.pipeline,
the rows whose options it touches run again, and every one of them must fail its comparison (profiles/pipeline_options.txt)."""
import numpy as np
import pytest
import torch

import pipeline_by_hand as BH
import pipeline_matrix as PM
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)

pytestmark = pytest.mark.gpu

_EXPECTED = {}                       # (pipeline, row, stream or clip) -> BH.Expected: computed once, shared with the mutants, never written


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expected(key, *args, **kw):
    if key not in _EXPECTED:
        _EXPECTED[key] = BH.by_hand(*args, **kw)
    return _EXPECTED[key]


def _net(d, hw):
    return ((hw[0] + 3) // 4 * 4, (hw[1] + 3) // 4 * 4) if PM.size_of(d)[1] else tuple(hw)


def _overlap(m, d, hw):
    """does the row's stream run the lagged schedule?  'default': from depth 2 on, where the ring engine serves the frame size"""
    want = PM.OVERLAPS[d["overlap"]]
    if want is None:
        return d["depth"] >= 2 and bool(m.overlap_available((4,) + _net(d, hw)))
    return want


def _manual_cuts(d, n):
    """two cut=True feeds, the second ``depth`` feeds behind the first"""
    if d["cuts"] != "manual":
        return []
    first = 1 if n <= 6 else 7
    return [first, first + d["depth"]]


def _live_streams(m, d):
    """-> [(picture size, frames, latency)] of the row's stream shape"""
    size = PM.size_of(d)[0]
    plan = {"A": [(size, None)], "B": [(size, 6), (size, None)], "C": [(size, None), (PM.other_size(d), None)]}[d["stream"]]
    out = []
    for hw, n in plan:
        latency = m.shift_num + d["depth"] - 1 + int(_overlap(m, d, hw))
        out.append((hw, n or latency + d["depth"] + 3, latency))
    return out


def _feed_stream(live, d, fr, hw, manual, exp, latency, fresh):
    """one stream through ``live`` against ``exp`` -> the frames it returned, stacked"""
    fmt, depth, n = d["pix_fmt"], d["depth"], fr.shape[0]
    mode = PM.SIGMAS[d["sigma"]][0]
    outs, nones = [], 0
    for k, f in enumerate(fr):
        r = live.feed(f, cut=True) if k in manual else live.feed(f)
        if k == 0:
            assert live.latency_final and live.latency == latency, (live.latency, latency)
        if r is None:
            nones += 1
        else:
            outs.append(r)
        j = k - (depth - 1)                               # the frame whose step this feed has waited for
        if mode == "auto":
            if j >= 0:
                assert live.last_sigma is not None and _bits(live.last_sigma) == _bits(exp.sigma[j]), ("last_sigma", k, live.last_sigma, exp.sigma[j])
            elif fresh:
                assert live.last_sigma is None
        elif mode == "nlf":
            assert live.last_sigma is None
            if j >= 0:
                assert live.last_noise_curve is not None and np.array_equal(_bits(live.last_noise_curve), _bits(exp.curves[j])), ("last_noise_curve", k)
            elif fresh:
                assert live.last_noise_curve is None
        else:
            assert live.last_sigma is None and live.last_noise_curve is None
        if d["cuts"] == "auto":
            assert live.last_cut_score == exp.scores[k] and bool(live.last_cut) == (k in exp.cuts), ("cut score", k, live.last_cut_score, exp.scores[k])
    assert nones == min(n, latency), (nones, latency)
    outs += live.flush()
    assert len(outs) == n
    assert all(o.dtype == fr.dtype and o.shape == fr.shape[1:] for o in outs)
    if mode == "auto":
        assert _bits(live.last_sigma) == _bits(exp.sigma[-1])
    if mode == "nlf":
        assert np.array_equal(_bits(live.last_noise_curve), _bits(exp.curves[-1]))
    got = np.stack(outs)
    if fmt in PM.ALPHA:
        assert np.array_equal(BH.alpha_of(fmt, got, hw), BH.alpha_of(fmt, fr, hw)), "alpha left its frame"
    bad = [t for t in range(n) if not np.array_equal(got[t], exp.out[t])]
    assert not bad, ("frames differ from the steps by hand", bad)
    return got


def run_live_row(m, i, anchor=False, fresh_object=False):
    """fresh_object: the second stream of shapes B and C is also run through an object of its own"""
    from bsvd_amd.pipeline import LiveStream
    d = PM.as_dict(PM.LIVE_ROWS[i], "live")
    fmt = d["pix_fmt"]
    live = LiveStream(m, **PM.constructor_kw(d, "live"))
    assert live.last_sigma is None and live.last_noise_curve is None and live.last_cut_score is None
    for si, (hw, n, latency) in enumerate(_live_streams(m, d)):
        fr = BH.frames(fmt, hw, n, seed=si, dark_from=n // 2 if d["cuts"] == "auto" else None, one_d=PM.one_d(d, "live"))
        manual = _manual_cuts(d, n)
        finds = hw[0] >= 16 and hw[1] >= 16               # a picture without a 16 x 16 block: every score 0.0, no cut, the frames of cuts=None
        exp = _expected(("live", i, si), m, d, fr, hw, cuts="auto" if d["cuts"] == "auto" else manual, want_cut=finds)
        if d["cuts"] == "auto" and not finds:
            assert exp.cuts == [] and all(v == 0.0 for v in exp.scores)
        if d["cuts"] == "manual":
            assert exp.cuts == manual and manual[1] - manual[0] <= d["depth"]
        if anchor:
            BH.anchor(d, fr, hw, exp)
        got = _feed_stream(live, d, fr, hw, manual, exp, latency, fresh=si == 0)
        if si == 1 and d["stream"] == "C":                # the rings were built again at the new size
            net = _net(d, hw)
            if fmt in PM.ALPHA:
                assert tuple(live._alpha.buf.shape[-2:]) == tuple(hw) and live._alpha.buf.shape[0] >= latency + d["depth"]
            if d["strength"] != "1":
                assert tuple(live._source.buf.shape[-2:]) == net and live._source.buf.shape[0] >= latency + d["depth"]
            if d["cuts"] == "auto":
                assert tuple(live._grids.shape[-2:]) == (hw[0] // 16, hw[1] // 16)
        if si == 1 and fresh_object:                      # the second stream is what a fresh object gives
            other = LiveStream(m, **PM.constructor_kw(d, "live", hw))
            again = [r for r in (other.feed(f, cut=True) if k in manual else other.feed(f) for k, f in enumerate(fr)) if r is not None]
            assert np.array_equal(np.stack(again + other.flush()), got)


def run_clip_row(m, i, anchor=False, table="clip"):
    from bsvd_amd.pipeline import ClipPipeline
    d = PM.as_dict(PM.ROWS[table][i], table)
    fmt, auto = d["pix_fmt"], d["cuts"] == "auto"
    size = PM.size_of(d)[0]
    finds = PM.finds_cuts(d)
    pipe = ClipPipeline(m, **PM.constructor_kw(d, table))
    clips, exps, f0 = [], [], 0
    for ci, T in enumerate(PM.CLIPS[d["clips"]]):
        fr = BH.frames(fmt, size, T, seed=10 + ci, dark_from=(T + 1) // 2 if auto and T >= 2 else None, one_d=PM.one_d(d, table))
        exp = _expected((table, i, ci), m, d, fr, size, cuts="auto" if auto else None, frame0=f0, want_cut=finds and T >= 2)
        if anchor:
            BH.anchor(d, fr, size, exp, frame0=f0)
        clips.append(fr)
        exps.append(exp)
        f0 += T
    seen = []

    def feeder():                                          # run() asks for clip k + 1 after it has submitted clip k
        for k, c in enumerate(clips):
            if k:
                seen.append(pipe.last_cuts)
            yield c
    got = list(pipe.run(feeder()))
    seen.append(pipe.last_cuts)
    assert len(got) == len(clips)
    if auto:
        assert seen == [e.cuts for e in exps], (seen, [e.cuts for e in exps])
        if finds:
            assert any(e.cuts for e in exps) and all(0 not in e.cuts for e in exps)
        else:                                              # no detector block: last_cuts == [] for every clip, every score 0.0
            assert seen == [[]] * len(clips) and all(v == 0.0 for e in exps for v in e.scores)
    else:
        assert seen == [None] * len(clips)
    for k, (g, c, e) in enumerate(zip(got, clips, exps)):
        assert g.dtype == c.dtype and g.shape == c.shape
        if fmt in PM.ALPHA:
            assert np.array_equal(BH.alpha_of(fmt, g, size), BH.alpha_of(fmt, c, size)), ("alpha left its clip", k)
        assert np.array_equal(g, e.out), ("clip differs from the steps by hand", k)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------
def _id(row):
    return "-".join(str(v) for v in row)


@pytest.mark.parametrize("i", range(len(PM.LIVE_ROWS)), ids=[_id(r) for r in PM.LIVE_ROWS])
def test_live_stream_row(model, i):     # noqa: F811
    run_live_row(model, i, anchor=True, fresh_object=True)


@pytest.mark.parametrize("i", range(len(PM.CLIP_ROWS)), ids=[_id(r) for r in PM.CLIP_ROWS])
def test_clip_pipeline_row(model, i):     # noqa: F811
    run_clip_row(model, i, anchor=True)


@pytest.mark.parametrize("i", range(len(PM.CLIP2_ROWS)), ids=[_id(r) for r in PM.CLIP2_ROWS])
def test_clip_pipeline_row_of_the_second_table(model, i):     # noqa: F811
    run_clip_row(model, i, anchor=True, table="clip2")


def test_feed_refuses_cut_true_under_auto_cuts_and_leaves_the_stream_as_it_was(model):     # noqa: F811
    """the one rule of the issue's list that no row can ask for (the cuts factor has one value per row): feed(frame, cut=True) raises under
    cuts='auto', before anything is enqueued, and the stream goes on to give the by-hand bytes"""
    from bsvd_amd.pipeline import LiveStream
    d = PM.as_dict(("bgra", "16x24", "const", "auto", "1", "none", 2, "default", "default", "none", "A"), "live")
    assert PM.valid(d, "live")
    live = LiveStream(model, **PM.constructor_kw(d, "live"))
    fr = BH.frames("bgra", (16, 24), 8, seed=0, dark_from=4)
    with pytest.raises(ValueError, match="cuts='auto'"):
        live.feed(fr[0], cut=True)
    assert live.count == 0 and not live.inflight and live.slots is None
    assert live.feed(fr[0]) is None and live.feed(fr[1]) is None
    with pytest.raises(ValueError, match="cuts='auto'"):
        live.feed(fr[2], cut=True)
    assert live.count == 2
    for f in fr[2:]:
        live.feed(f)
    exp = BH.by_hand(model, d, fr, (16, 24), cuts="auto")
    assert exp.cuts == [4] and np.array_equal(np.stack(live.flush()), exp.out)


def test_the_frames_are_coloured_and_every_frame_has_a_noise_level_of_its_own(model):     # noqa: F811
    """what the rows rest on: R, G, B planes that differ, both ends of the code range, alpha over its range, and per-frame estimates that
    differ from frame to frame -- a stale dev_sigma / dev_curve shows"""
    d = PM.as_dict(PM.LIVE_ROWS[0], "live")
    hw = PM.size_of(d)[0]
    fr = BH.frames("rgba64le", hw, 12, seed=0)
    assert not fr.flags.writeable and fr.min() == 0 and fr.max() == 65535
    assert not np.array_equal(fr[..., 0], fr[..., 1]) and not np.array_equal(fr[..., 1], fr[..., 2])
    a = BH.alpha_of("rgba64le", fr, hw)
    assert a.min() == 0 and a.max() == 65535
    exp = BH.by_hand(model, d, fr, hw)
    assert len({c.tobytes() for c in exp.curves}) == 12
    e2 = BH.by_hand(model, dict(d, sigma="auto"), fr, hw)
    assert len(set(e2.sigma.tolist())) == 12
    nv = BH.frames("p010", hw, 3, seed=0)
    Y, Cb, Cr, _ = BH.Y2.unpack(BH.as_bytes(nv), hw[0], hw[1], "p010", (hw[1] + PM.PITCH_EXTRA) * 2)
    assert Y.min() == 0 and Y.max() == 1023 and abs(Cb.mean() - 512) > 40 and abs(Cr.mean() - 512) > 40 and not np.array_equal(Cb, Cr)


@pytest.mark.parametrize("i", [0, 1])
def test_the_anchor_fails_a_by_hand_side_that_is_one_step_off(model, i):     # noqa: F811
    """the numpy anchor is a check, not a formality: the mandatory rows' by-hand results with one sample of the surface moved by two codes,
    with one element of the noise plane one ulp up, and with the curves of two frames swapped, each fail it"""
    d = PM.as_dict(PM.LIVE_ROWS[i], "live")
    hw = PM.size_of(d)[0]
    fr = BH.frames(d["pix_fmt"], hw, 6, seed=0, dark_from=3 if d["cuts"] == "auto" else None, one_d=PM.one_d(d, "live"))
    exp = BH.by_hand(model, d, fr, hw, cuts="auto" if d["cuts"] == "auto" else [1, 4])
    BH.anchor(d, fr, hw, exp)
    out = exp.out.copy()
    out.reshape(-1)[5] = (int(out.reshape(-1)[5]) + (128 if out.dtype == np.uint16 else 2)) % 65536      # p010: two codes of the high ten bits
    with pytest.raises(AssertionError, match="encode"):
        BH.anchor(d, fr, hw, exp._replace(out=out))
    x = exp.x.clone()
    x[2, 3, 1, 1] = torch.nextafter(x[2, 3, 1, 1], x.new_tensor(1.0))
    with pytest.raises(AssertionError, match="map model"):
        BH.anchor(d, fr, hw, exp._replace(x=x))
    with pytest.raises(AssertionError, match="curve model"):
        BH.anchor(d, fr, hw, exp._replace(curves=exp.curves[::-1].copy()))
    y = exp.y.clone()
    y[0, 1] += 0.01
    with pytest.raises(AssertionError, match="encode"):
        BH.anchor(d, fr, hw, exp._replace(y=y))


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------
def _effective_overlap(d):
    return d["overlap"] == "on" or (d["overlap"] == "default" and d["depth"] >= 2)


def _m_source_ring_behind(mp, P):
    def next_out(self):
        if self.emitted >= self.fed:
            raise RuntimeError("source ring: frame %d comes out before it went in" % self.emitted)
        self.emitted += 1
        return self.buf[(self.emitted - 2) % self.buf.shape[0]]
    mp.setattr(P._SourceRing, "next_out", next_out)


def _m_alpha_reset_noop(mp, P):
    mp.setattr(P._AlphaRing, "reset", lambda self: None)


def _sticky_finish(P):
    class Finish(P._Finish):
        """``emitted`` cannot be set back to 0 once it has counted"""
        @property
        def emitted(self):
            return self.__dict__.get("_emitted", 0)

        @emitted.setter
        def emitted(self, v):
            if v != 0:
                self.__dict__["_emitted"] = v
    return Finish


def _m_emitted_not_reset(mp, P):
    mp.setattr(P, "_Finish", _sticky_finish(P))


def _m_scene_not_forgotten(mp, P):
    flush = P.LiveStream.flush

    def mutant(self):
        self._forget_scene = lambda: None
        try:
            return flush(self)
        finally:
            del self._forget_scene
    mp.setattr(P.LiveStream, "flush", mutant)


def _m_nlf_gain_dropped(mp, P):
    est = P.estimate_noise_curve
    mp.setattr(P, "estimate_noise_curve", lambda x, picture=None, gain=1.0: est(x, picture=picture))


def _m_cut_dropped_when_overlap(mp, P):
    step, detect = P.LiveStream._step, P.LiveStream._detect

    def _step(self, frame_u8, last=False, cut=False):
        return step(self, frame_u8, last=last, cut=cut and not self.overlap)

    def _detect(self, slot):
        x, cut = detect(self, slot)
        return x, cut and not self.overlap
    mp.setattr(P.LiveStream, "_step", _step)
    mp.setattr(P.LiveStream, "_detect", _detect)


def _m_curve_of_wrong_slot(mp, P):
    pop = P.LiveStream._pop

    def _pop(self):
        slot, _, has_sigma = self.inflight[0]
        other = self.slots[(self.slots.index(slot) - 1) % len(self.slots)]
        r = pop(self)
        if has_sigma and self.nlf_sigma:
            self.last_noise_curve = [float(v) for v in other.side["curve"].pin]
        return r
    mp.setattr(P.LiveStream, "_pop", _pop)


def _m_clip_frame0_zero(mp, P):
    class Finish(P._Finish):
        def dither_kw(self, frames):
            kw = super().dither_kw(frames)
            return dict(kw, frame0=0) if kw else kw
    mp.setattr(P, "_Finish", Finish)


def _m_clip_alpha_of_the_clip_before(mp, P):
    to_output, state = P._RgbSurface.to_output, {}

    def mutant(self, y, geom, alpha=None, **dither):
        prev, use = state.get("prev"), alpha
        if alpha is not None and prev is not None and prev.shape[0] >= alpha.shape[0] and prev.shape[1:] == alpha.shape[1:]:
            use = prev[:alpha.shape[0]].contiguous()      # as many planes of the clip before as this clip has frames: inside both buffers
        state["prev"] = alpha
        return to_output(self, y, geom, alpha=use, **dither)
    mp.setattr(P._RgbSurface, "to_output", mutant)


MUTANTS = {
    "source_ring_one_slot_behind": ("live", _m_source_ring_behind, lambda d: d["strength"] != "1"),
    "finish_emitted_not_reset_by_flush": ("live", _m_emitted_not_reset,
                                          lambda d: d["dither"] == "random" and d["stream"] in "BC" and d["strength"] != "0"),
    "scene_not_forgotten_by_flush": ("live", _m_scene_not_forgotten, lambda d: PM.finds_cuts(d) and d["stream"] == "B"),
    "nlf_branch_drops_sigma_gain": ("live", _m_nlf_gain_dropped, lambda d: d["sigma"] == "nlf*0.8"),
    "step_drops_cut_when_overlap": ("live", _m_cut_dropped_when_overlap,
                                    lambda d: (d["cuts"] == "manual" or PM.finds_cuts(d)) and _effective_overlap(d) and d["strength"] != "0"),
    "pop_reads_pin_curve_of_the_wrong_slot": ("live", _m_curve_of_wrong_slot, lambda d: d["sigma"] in ("nlf", "nlf*0.8") and d["depth"] >= 2),
    "clip_frame0_is_zero_for_every_clip": ("clip", _m_clip_frame0_zero, lambda d: d["dither"] == "random" and d["strength"] != "0"),
    "clip_gets_the_alpha_of_the_clip_before": ("clip", _m_clip_alpha_of_the_clip_before, lambda d: d["pix_fmt"] in PM.ALPHA),
}


def _rows_touched(pipeline, touches):
    """-> [(table, row)]; a ClipPipeline fault meets the rows of both ClipPipeline tables"""
    tables = ("live",) if pipeline == "live" else ("clip", "clip2")
    return [(t, i) for t in tables for i, r in enumerate(PM.ROWS[t]) if touches(PM.as_dict(r, t))]


def _survivors_and_killers(m, mp, name, rows):
    from bsvd_amd import pipeline as P
    pipeline, patch, _ = MUTANTS[name] if name in MUTANTS else ("live", _m_alpha_reset_noop, None)
    patch(mp, P)
    killed, why = [], []
    try:
        for t, i in rows:
            try:
                if t == "live":
                    run_live_row(m, i)
                else:
                    run_clip_row(m, i, table=t)
            except AssertionError as e:
                killed.append((t, i))
                why.append(str(e).split("\n")[0][:100])
    finally:
        mp.undo()
        torch.cuda.synchronize()
    fmt = lambda rs: " ".join("%s:%d" % r for r in rs)
    print("mutant %s: rows run [%s], killed by [%s] %s" % (name, fmt(rows), fmt(killed), sorted(set(why))))
    return killed


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_killed_by_matrix_rows(model, monkeypatch, name):     # noqa: F811
    """the rows whose option values the fault touches, run again with the fault in place: every one of them fails its comparison (the
    killing rows are printed, and recorded in profiles/pipeline_options.txt).  strength = 0 returns the source whatever the network saw and
    moves no whole code under dither: those rows cannot see a lost cut or a wrong dither index, and are not counted as touched; nor is
    a cuts='auto' row whose picture holds no detector block.  The expected bytes come from pipeline_by_hand, which uses nothing of
    bsvd_amd.pipeline: no mutant reaches them."""
    pipeline, _, touches = MUTANTS[name]
    rows = _rows_touched(pipeline, touches)
    assert rows, "no row of the table touches the fault"
    killed = _survivors_and_killers(model, monkeypatch, name, rows)
    assert killed, "the fault changed no compared value"
    assert killed == rows, ("rows the fault touches and that did not see it", sorted(set(rows) - set(killed)))


def test_alpha_ring_reset_as_a_no_op_changes_nothing_a_caller_can_see(model, monkeypatch):     # noqa: F811
    """``_AlphaRing.reset`` as a no-op is an equivalent mutant, not a survivor: flush() drains every step, so ``fed == emitted`` when it
    resets them, and planes written at (fed - 1) % N are read at (emitted - 1) % N whatever the common offset; a new frame size builds a new
    ring.  Shown here rather than supposed: the counters are equal after every flush, and the alpha rows with a second stream pass with
    the reset removed."""
    from bsvd_amd.pipeline import LiveStream
    rows = _rows_touched("live", lambda d: d["pix_fmt"] in PM.ALPHA and d["stream"] in "BC")
    assert rows
    assert _survivors_and_killers(model, monkeypatch, "alpha_ring_reset_is_a_no_op", rows) == []
    monkeypatch.setattr("bsvd_amd.pipeline._AlphaRing.reset", lambda self: None)
    live = LiveStream(model, sigma=30 / 255.0, depth=2, pix_fmt="bgra")
    fr = BH.frames("bgra", (16, 24), 5, seed=0)
    for f in fr:
        live.feed(f)
    assert len(live.flush()) == 5 and live._alpha.fed == live._alpha.emitted == 5
