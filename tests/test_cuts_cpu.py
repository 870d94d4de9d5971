"""Scene cuts in the stream schedules, on the CPU through the oracle-backed executor, and the numpy model of the cut detector.

The contract: with the scene starts given, every schedule computes what each scene computes when it is run alone -- bit for bit, since a
cut is nothing but the zeros a clip's ends get (halo None), placed in mid-stream.  The clip has a one-frame scene, a two-frame scene, scenes
shorter than the 16-step pipeline and a longer one; two cuts are always inside the pipeline at once.  The scenes differ by O(1), so a leak
across a cut is far above rounding."""
import numpy as np
import pytest
import torch

import scene_model
from helpers import bsvd_keys
from oracle_exec import OracleExecutor
from seeded import seeded_state, seeded_clip
from bsvd_amd import schedule
from bsvd_amd.netspec import make_netspec
from bsvd_amd.schedule import StreamPipeline
from bsvd_amd.stream_plan import StreamEngine

CHNS = [32, 64, 128]
H, W = 16, 24
LENGTHS = (5, 1, 2, 19, 13)
STARTS = tuple(int(v) for v in np.cumsum((0,) + LENGTHS[:-1]))          # 0, 5, 6, 8, 27
T = sum(LENGTHS)


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _scenes(starts=STARTS, n=T):
    edges = sorted(set(starts) | {0}) + [n]
    return list(zip(edges[:-1], edges[1:]))


def _pipeline(net, st, chunks, flags=None):
    """the allocating StreamPipeline over a list of chunks ([n,C,H,W] each)"""
    ex, pipe = OracleExecutor(st), StreamPipeline(net)
    ypl = (net.out_ch, None)
    outs = []
    for k, c in enumerate(chunks):
        outs.append(pipe.feed(ex, c, x_planar=True, y_planar=ypl) if flags is None else
                    pipe.feed(ex, c, x_planar=True, y_planar=ypl, cut=flags[k]))
    while len(outs) < len(chunks) + pipe.shift_num:
        outs.append(pipe.feed(ex, None, x_planar=True, y_planar=ypl))
    assert all(o is None for o in outs[:pipe.shift_num]) and all(o is not None for o in outs[pipe.shift_num:])
    assert not pipe.cuts.pending
    return torch.cat(outs[pipe.shift_num:])


def _split(x, chunk, starts):
    """(chunks, flags): no chunk spans a scene start"""
    chunks, flags = [], []
    for a, b in _scenes(starts, x.shape[0]):
        for i in range(a, b, chunk):
            chunks.append(x[i:min(i + chunk, b)])
            flags.append(i == a and a in starts)
    return chunks, flags


@pytest.fixture(scope="module")
def case(_one_thread):
    """(net, state, clip, per-scene reference): computed once, shared, never written to"""
    net = make_netspec(CHNS, CHNS[0], 4, 3, "relu6", CHNS[0])
    st = seeded_state(bsvd_keys(CHNS, CHNS[0], 4, 3, CHNS[0]), 5)
    x = torch.from_numpy(seeded_clip((1, T, 4, H, W), 6, kind="sigma30"))[0].clone()
    for k, (a, b) in enumerate(_scenes()):
        x[a:b, :3] += float(k)                                          # scene k + k: the scenes differ by O(1)
    want = torch.cat([_pipeline(net, st, list(x[a:b].split(1))) for a, b in _scenes()])
    return net, st, x, want


def _engine(net, st, chunk=1, poison=True):
    return StreamEngine(net, OracleExecutor(st), H, W, 4, chunk=chunk, alloc=lambda shape: torch.zeros(shape, dtype=torch.float32), poison=poison)


def _cp(y):
    return None if y is None else y.clone()


def _run_feed(eng, chunks, flags, kw=True):
    ypl, shift = (eng.net.out_ch, None), eng.net.shift_num
    outs = []
    for c, f in zip(chunks, flags or [False] * len(chunks)):
        outs.append(_cp(eng.feed(c, ypl, cut=f) if kw else eng.feed(c, ypl)))
    while len(outs) < len(chunks) + shift:
        outs.append(_cp(eng.feed(None, ypl)))
    assert eng.feed(None, ypl) is None
    assert all(o is None for o in outs[:shift]) and all(o is not None for o in outs[shift:])       # no step emits None because of a cut
    assert not eng.cuts.pending
    eng.clear()
    return torch.cat(outs[shift:])


def _run_lagged(eng, chunks, flags, kw=True):
    ypl, shift = (eng.net.out_ch, None), eng.net.shift_num
    outs = []
    for k in range(len(chunks) + shift + 1):
        c = chunks[k] if k < len(chunks) else None
        y = _cp(eng.feed_lagged(c, ypl, cut=flags[k]) if kw and c is not None else eng.feed_lagged(c, ypl))
        if k >= 1:
            outs.append(y)
    assert eng.feed_lagged(None, ypl, last=True) is None
    assert all(o is None for o in outs[:shift]) and all(o is not None for o in outs[shift:])
    assert not eng.cuts.pending
    eng.clear()
    return torch.cat(outs[shift:])


# ------------------------------------------------------------------------------------------------ schedules
def test_the_scenes_are_told_apart_by_the_reference(case):
    """the clip can tell: run as ONE scene it differs from the per-scene result on both sides of every cut"""
    net, st, x, want = case
    whole = _pipeline(net, st, list(x.split(1)))
    for s in STARTS[1:]:
        assert not torch.equal(whole[s - 1], want[s - 1]) and not torch.equal(whole[s], want[s])
        assert float((whole[s] - want[s]).abs().max()) > 1e-3


def test_stream_pipeline_with_flags(case):
    net, st, x, want = case
    chunks, flags = _split(x, 1, STARTS[1:])
    assert torch.equal(_pipeline(net, st, chunks, flags), want)


@pytest.mark.parametrize("run", [_run_feed, _run_lagged])
def test_stream_engine_with_flags(case, run):
    net, st, x, want = case
    chunks, flags = _split(x, 1, STARTS[1:])
    eng = _engine(net, st)
    got = run(eng, chunks, flags)
    assert not torch.isnan(got).any() and torch.equal(got, want)
    n = len(eng.plans)
    assert torch.equal(run(eng, chunks, flags), want) and len(eng.plans) == n           # the same cut phases again: every plan was seen


@pytest.mark.parametrize("run", [_run_feed, _run_lagged])
def test_scene_aligned_chunks_of_two(case, run):
    """a scene's last chunk is short in mid-stream (scenes of 5, 1, 19 and 13 frames); reference: the allocating pipeline over each scene's
    own chunks (the CPU comparator is not batch invariant, so chunks are compared with chunks; the GPU test compares with clip_forward)"""
    net, st, x, _ = case
    want = torch.cat([_pipeline(net, st, _split(x[a:b], 2, ())[0]) for a, b in _scenes()])
    chunks, flags = _split(x, 2, STARTS[1:])
    assert {c.shape[0] for c in chunks[:-1]} == {1, 2}
    got = run(_engine(net, st, chunk=2), chunks, flags)
    assert not torch.isnan(got).any() and torch.equal(got, want)


@pytest.mark.parametrize("run", [_run_feed, _run_lagged])
@pytest.mark.parametrize("starts", [(), (0,)])
def test_no_cut_changes_no_plan_and_no_bit(case, run, starts):
    net, st, x, _ = case
    chunks = list(x[:30].split(1))
    plain = _engine(net, st)
    want = run(plain, chunks, None, kw=False)
    eng = _engine(net, st)
    got = run(eng, chunks, [i in starts for i in range(30)])
    assert torch.equal(got, want)
    # same rings allocated in the same order would not give the same addresses: compare the keys with the addresses taken relative to each ring
    assert list(eng.plans.keys()) != [] and len(eng.plans) == len(plain.plans)
    assert _relative(eng) == _relative(plain)


def _relative(eng):
    """eng.plans' keys with every address replaced by (ring, byte offset into it)"""
    bases = sorted((ring[0].data_ptr(), key) for key, ring in eng.rings.items())

    def rel(p):
        if p == 0:
            return 0
        base, key = max(b for b in bases if b[0] <= p)
        return key, p - base
    return [tuple((r[0], r[1]) + tuple(rel(p) for p in r[2:]) for r in (sig[1] if sig and sig[0] == "shared" else sig)) for sig in eng.plans]


# ------------------------------------------------------------------------------------------------ mutants
class _IgnorePrev(schedule._TsmStage):
    """forgets that its pending frame starts a scene (prev side) but sees the flag of the frame coming in (next side)"""

    def feed(self, ex, nxt):
        if self.mid is not None:
            self.mid_cut = False
        return super().feed(ex, nxt)


class _IgnoreNext(schedule._TsmStage):
    """sees the flag of its pending frame (prev side) but not of the frame coming in (next side)"""

    def feed(self, ex, nxt):
        if self.mid is None or nxt is None:
            return super().feed(ex, nxt)
        real, self.cuts = self.cuts, None
        try:
            y = super().feed(ex, nxt)
        finally:
            self.cuts = real
        self.mid_cut = bool(real) and (self.n_seen - 1) in real
        return y


@pytest.mark.parametrize("run", [_run_feed, _run_lagged])
@pytest.mark.parametrize("mutant", [_IgnorePrev, _IgnoreNext])
def test_one_sided_mutants_are_caught(case, monkeypatch, mutant, run):
    net, st, x, want = case
    monkeypatch.setattr(schedule, "_TsmStage", mutant)
    eng = _engine(net, st, poison=False)
    monkeypatch.undo()
    assert all(type(s) is mutant for s in eng.t1.stage.values())
    ypl, shift = (net.out_ch, None), net.shift_num
    chunks, flags = _split(x, 1, STARTS[1:])
    outs = []
    if run is _run_feed:
        for c, f in zip(chunks, flags):
            outs.append(_cp(eng.feed(c, ypl, cut=f)))
        for _ in range(shift):
            outs.append(_cp(eng.feed(None, ypl)))
    else:
        for k in range(len(chunks) + shift + 1):
            y = _cp(eng.feed_lagged(chunks[k], ypl, cut=flags[k]) if k < len(chunks) else eng.feed_lagged(None, ypl))
            if k >= 1:
                outs.append(y)
    got = torch.cat(outs[shift:])
    assert got.shape == want.shape and not torch.equal(got, want)
    for s in STARTS[1:]:
        side = s if mutant is _IgnorePrev else s - 1                 # the frame that reads across the cut
        assert float((got[side] - want[side]).abs().max()) > 1e-3
    print("%s / %s: max-abs %.3g" % (mutant.__name__, run.__name__, float((got - want).abs().max())))


def test_flag_one_frame_late_at_denblock_2_is_caught(case):
    """the lagged schedule hands DenBlock 1's frames to DenBlock 2 one step later; a flag that is handed over with the step rather than
    with the frame (here: DenBlock 2 looks up an index one too high) cuts in the wrong place"""
    net, st, x, want = case
    eng = _engine(net, st, poison=False)
    late = set()
    for s in eng.t2.stage.values():
        s.cuts = late
    ypl, shift = (net.out_ch, None), net.shift_num
    chunks, flags = _split(x, 1, STARTS[1:])
    outs = []
    for k in range(len(chunks) + shift + 1):
        if k < len(chunks) and flags[k]:
            late.add(k + 1)
        y = _cp(eng.feed_lagged(chunks[k], ypl, cut=flags[k]) if k < len(chunks) else eng.feed_lagged(None, ypl))
        if k >= 1:
            outs.append(y)
    got = torch.cat(outs[shift:])
    assert got.shape == want.shape and not torch.equal(got, want)
    assert float((got[STARTS[-1]] - want[STARTS[-1]]).abs().max()) > 1e-3


def test_clear_forgets_pending_cuts(case):
    net, st, x, want = case
    eng = _engine(net, st)
    for t in range(7):
        eng.feed(x[t:t + 1], (3, None), cut=t in (5, 6))
    assert eng.cuts.pending == {5, 6}
    eng.clear()
    assert not eng.cuts.pending and eng.cuts.n_in == 0
    chunks, flags = _split(x, 1, STARTS[1:])
    assert torch.equal(_run_feed(eng, chunks, flags), want)


# ------------------------------------------------------------------------------------------------ the detector's model
def test_model_grid_by_hand():
    x = np.ones((1, 3, 32, 48), np.float32)
    g = scene_model.grid(x)
    assert g.shape == (1, 2, 3) and (g == 256 * 1020).all()
    x = np.zeros((1, 4, 32, 48), np.float32)
    x[0, 1, 17, 33] = 0.5                                   # 127.5 -> 128 (round half to even); G counts twice
    x[0, 3] = 1.0                                           # the sigma plane is not read
    g = scene_model.grid(x)
    assert g[0, 1, 2] == 256 and g.sum() == 256
    x[0, 0, 0, 0], x[0, 2, 0, 1], x[0, 0, 0, 2] = np.nan, 7.0, -3.0
    assert scene_model.grid(x)[0, 0, 0] == 255
    assert scene_model.grid(np.ones((2, 3, 36, 52), np.float32), picture=(34, 50)).shape == (2, 2, 3)
    assert scene_model.grid(np.ones((2, 3, 8, 48), np.float32)).shape == (2, 0, 3)


def test_model_sad_and_score_rule_by_hand():
    g = np.array([[[10, 20]], [[13, 15]], [[13, 15]]])
    assert scene_model.sad(g).tolist() == [0, 8, 0]
    assert scene_model.sad(g, prev=np.array([[0, 0]])).tolist() == [30, 8, 0]
    assert scene_model.mafd([261120 * 6], 6)[0] == 100.0
    assert scene_model.mafd([5, 6], 0).tolist() == [0.0, 0.0]
    s = scene_model.scores([0.0, 1.0, 33.0, 1.0, 30.0, 31.0])
    assert s.tolist() == [0.0, 1.0, 32.0, 1.0, 29.0, 1.0]
    assert scene_model.scores([5.0], prev_mafd=4.0).tolist() == [1.0]


@pytest.mark.parametrize("size", [(64, 96), (128, 192)])
def test_detection_margins_on_the_model(size):
    """E|a - b| = 1/3 for two uniform values: mafd ~ 33 at a cut, ~ 0.9 (noise of sigma 50 averaged over 256 pixels) elsewhere"""
    x, starts = scene_model.margin_clip(*size, seed=size[0])
    found, s = scene_model.cuts(x)
    print(size, "scene starts:", [round(float(s[t]), 2) for t in starts[1:]], "others: max %.2f" % max(s[t] for t in range(len(s)) if t not in starts))
    for t in range(len(s)):
        if t in starts[1:]:
            assert s[t] >= 2 * 10.0
        else:
            assert s[t] <= 0.5 * 10.0
    assert found == starts[1:]


# ------------------------------------------------------------------------------------------------ validation
def test_cut_without_a_frame_is_refused(case):
    net, st, x, _ = case
    eng = _engine(net, st)
    with pytest.raises(ValueError, match="frame"):
        eng.feed(None, (3, None), cut=True)
    with pytest.raises(ValueError, match="frame"):
        StreamPipeline(net).feed(OracleExecutor(st), None, cut=True)
    eng.clear()
    with pytest.raises(ValueError, match="frame"):
        eng.feed_lagged(None, (3, None), cut=True)


@pytest.mark.parametrize("bad", [[40], [-1], [True], [3.0], [np.float32(2)], "auto", [None]])
def test_check_cuts_refuses(bad):
    from bsvd_amd.arch import check_cuts
    with pytest.raises(ValueError, match="cut"):
        check_cuts(bad, 40)


def test_check_cuts_accepts():
    from bsvd_amd.arch import check_cuts
    assert check_cuts(None, 5) == [] and check_cuts([0], 5) == [] and check_cuts((3, np.int64(1), 3, 0), 5) == [1, 3]
    assert check_cuts(iter({4}), 5) == [4]


def _model():
    import bsvd_amd
    return bsvd_amd.BSVD(chns=CHNS, mid_ch=CHNS[0], norm="none", act="relu6", interm_ch=CHNS[0], pretrain_ckpt=None).eval()


def test_model_api_refuses_before_any_launch():
    """every check comes before the device is asked for (there is none here: reaching it would raise RuntimeError)"""
    m = _model()
    x = torch.zeros((1, 6, 4, 8, 8))
    for bad in ([6], [-1], [True], [2.0]):
        with pytest.raises(ValueError, match="cut"):
            m.forward(x, cuts=bad)
        with pytest.raises(ValueError, match="cut"):
            m.streaming_forward(x[0], cuts=bad)
        with pytest.raises(ValueError, match="cut"):
            m.clip_forward(x[0], cuts=bad)
    with pytest.raises(ValueError, match="halo_fn and cuts"):
        m.clip_forward(x[0], halo_fn=lambda sp, v: (None, None), cuts=[3])
    with pytest.raises(ValueError, match="cut=True needs a frame"):
        m.feedin_one_element(None, cut=True)
    with pytest.raises(ValueError, match="cut=True needs a frame"):
        m.feed_overlapped(None, cut=True)
    with pytest.raises(ValueError, match="cut=True needs a frame"):
        m.feed_overlapped(x[0, :1], last=True, cut=True)
    with pytest.raises(RuntimeError, match="HIP device"):                  # valid cuts go on to the device
        m.forward(x, cuts=[0, 3])


class _FakeModel:
    """what the pipelines' constructors look at before they touch a device"""

    class net:
        net_in_ch = 4

    def _device(self):
        raise AssertionError("the cuts check comes before the device")


@pytest.mark.parametrize("which", ["ClipPipeline", "LiveStream"])
def test_pipelines_refuse_at_construction(which):
    from bsvd_amd import pipeline
    cls = getattr(pipeline, which)
    for bad in ("automatic", True, [3], 5):
        with pytest.raises(ValueError, match="cuts must be None or 'auto'"):
            cls(_FakeModel(), sigma=0.1, cuts=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "ten", None, True):
        with pytest.raises(ValueError, match="cut_threshold"):
            cls(_FakeModel(), sigma=0.1, cuts="auto", cut_threshold=bad)
    with pytest.raises(AssertionError, match="before the device"):
        cls(_FakeModel(), sigma=0.1, cuts="auto", cut_threshold=12)


def test_live_stream_refuses_a_flag_in_auto_mode():
    from bsvd_amd.pipeline import LiveStream
    live = LiveStream.__new__(LiveStream)
    live.auto_cuts = True
    with pytest.raises(ValueError, match="finds the cuts itself"):
        live.feed(np.zeros((8, 8, 3), np.uint8), cut=True)


def test_frame_io_refuses():
    from bsvd_amd import frame_io
    for x in (None, torch.zeros(1, 4, 32, 32), torch.zeros(4, 32, 32)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            frame_io.scene_scores(x)
        with pytest.raises(ValueError, match="float32 device tensor"):
            frame_io.scene_cuts(x)
    with pytest.raises(ValueError, match="cut_threshold"):
        frame_io.scene_cuts(None, threshold=0)
    score, mafd = frame_io.cut_scores([0, 261120 * 6, 0], 6)
    assert mafd == [0.0, 100.0, 0.0] and score == [0.0, 100.0, 0.0]
    assert frame_io.cut_scores([5], 0) == ([0.0], [0.0])
    assert frame_io.cut_scores([261120 * 3], 6, prev_mafd=45.0) == ([5.0], [50.0])


def test_entry_points_validate_without_a_device():
    import ctypes
    from bsvd_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    x = ctypes.addressof(buf)
    out = (ctypes.c_int64 * 8)()
    o = ctypes.addressof(out)

    def err():
        return lib.bsvd_last_error().decode()

    assert {"bsvd_scene_grid", "bsvd_scene_diff"} <= set(_lib.EXPORTS)
    for args, word in (((None, 1, 32, 32, 32, 32, 3 * 1024, o, None), "x is NULL"), ((x + 2, 1, 32, 32, 32, 32, 3 * 1024, o, None), "4-byte"),
                       ((x, 0, 32, 32, 32, 32, 3 * 1024, o, None), "frames"), ((x, -2, 32, 32, 32, 32, 3 * 1024, o, None), "frames"),
                       ((x, 1, -1, 32, 32, 32, 3 * 1024, o, None), "H ="), ((x, 1, 32, -16, 32, 32, 3 * 1024, o, None), "W ="),
                       ((x, 1, 32, 32, 16, 32, 3 * 1024, o, None), "Hp"), ((x, 1, 32, 32, 32, 0, 3 * 1024, o, None), "Wp"),
                       ((x, 1, 32, 32, 32, 32, 3 * 1024 - 1, o, None), "frame_stride"), ((x, 1, 32, 32, 32, 32, 3 * 1024, None, None), "grid is NULL")):
        assert lib.bsvd_scene_grid(*args) == -3 and word in err(), (args, err())
    assert lib.bsvd_scene_grid(x, 1, 8, 48, 8, 48, 3 * 8 * 48, None, None) == 0          # GH = 0: valid, nothing to launch
    assert lib.bsvd_scene_grid(x, 3, 15, 15, 16, 16, 4 * 256, None, None) == 0
    for args, word in (((o, None, 0, 6, o, None), "frames"), ((o, None, 70000, 6, o, None), "frames"), ((o, None, 1, -1, o, None), "blocks"),
                       ((o, None, 1, 6, None, None), "sad is NULL"), ((o, None, 1, 6, o + 4, None), "8-byte"), ((None, None, 1, 6, o, None), "grid is NULL"),
                       ((o, o + 2, 1, 6, o, None), "4-byte")):
        assert lib.bsvd_scene_diff(*args) == -3 and word in err(), (args, err())
