"""Live-stream soak on the MI355X (VERDICT "next round" item 6): streams of a thousand frames and more through ``feedin_one_element``,
``feed_overlapped``, ``streaming_forward`` and ``pipeline.LiveStream``, checked against SHORT clips (tests/soak.py: output frame t depends
on input frames t - shift_num ... t + shift_num only, so the clip schedule over that window IS frame t, bit for bit; the premise and the
comparator's teeth are tests/test_soak_cpu.py).  Beside the frames: the steady state captures no graph, makes no plan, launches nothing
layer by layer, holds torch's allocator at the same byte count at every step; build / release cycles give the memory back; two host
threads with a model and a HIP stream each get their solo frames; graph eviction keeps streaming.

Frame counts are conditions, not measurements: the short form (what the suite runs) feeds >= 1000 steady-state frames (100 ring periods)
at 36 x 52 -- half and quarter resolution 18 x 26 and 9 x 13, ragged and odd against every tile -- and >= 300 at 128 x 192 (every layer
on more than one tile).  BSVD_SOAK_LONG=1 adds the long form, run by hand: 20 000 frames at 128 x 192 and 2 000 at 540 x 960.
Every case prints one ``SOAK`` line (frames, wall time, final counts); profiles/stream_soak.txt holds a run's.

How graphs come to be decides what a repeated stream may add: a step's plans are issued directly at the first sighting of its key and
captured at the SECOND (stream_plan.StreamEngine._issue).  A second identical stream therefore still captures the keys its first run met
once (pipeline fill and flush) but launches nothing directly and plans nothing; from the third on nothing at all is added.
"""
import gc
import os
import threading
import time

import numpy as np
import pytest
import torch

import soak
from helpers import bsvd_keys
from seeded import seeded_state

pytestmark = pytest.mark.gpu

LONG = os.environ.get("BSVD_SOAK_LONG", "0") == "1"
SMALL, LARGE = (36, 52), (128, 192)
C64 = dict(chns=[64, 128, 256], mid_ch=64, interm_ch=64)


def _dev():
    return torch.device("cuda", 0)


def _state(seed):
    return seeded_state(bsvd_keys(C64["chns"], C64["mid_ch"], 4, 3, C64["interm_ch"]), seed)


def _model(precision="f16x3", seed=17, **kw):
    import bsvd_amd
    m = bsvd_amd.BSVD(norm="none", act="relu6", pretrain_ckpt=None, precision=precision, **C64, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state(seed).items()})
    return m.to(_dev()).eval()


def _frames(model, steady):
    """stream length with ``steady`` steady-state frames after soak.steady_start, ending off the ring period"""
    return soak.steady_start(model) + steady + 7


_POOLS = {}


def _pool(size, seed=3):
    """one pool per frame size, shared by every case, never written to"""
    if (size, seed) not in _POOLS:
        _POOLS[size, seed] = soak.Pool(4, size[0], size[1], seed, device=_dev(), sigma=30.0 / 255.0)
    return _POOLS[size, seed]


def _line(what, T, seconds, model, extra=""):
    eng = model._stream_eng
    return ("SOAK %-58s %6d frames %7.2f s  plans %3d graphs %3d captures %3d batch launches %3d replays %6d  allocated %d B%s"
          % (what, T, seconds, len(eng.plans), soak.real_graphs(eng), eng.stats["graph_captures"], eng.stats["batch_launches"],
             eng.stats["graph_replays"], torch.cuda.memory_allocated(), extra))


def _timed_stream(model, pool, api, T, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, log = soak.run_stream(model, pool, api, T, **kw)
    torch.cuda.synchronize()
    return got, log, time.perf_counter() - t0


# ---- a. long streams against their windows --------------------------------------------------------------------------------------------
# (precision, wide_conv, frame size, steady-state frames): models and expected frames are shared by the two apis of a configuration.
# Floors: 1000 at 36 x 52, 300 at 128 x 192; raised as far as a case stays within about three seconds on the MI355X (0.6 - 0.8 ms per
# feed in the split modes, 1.5 - 2.8 ms in exact fp32 at 36 x 52: profiles/stream_soak.txt)
_CONFIGS = {
    "f16x3": ("f16x3", "auto", SMALL, 3000),
    "fp32": ("fp32", "auto", SMALL, 1000),
    "f16": ("f16", "auto", SMALL, 3000),
    "f16x3-128x192": ("f16x3", "auto", LARGE, 2000),
    "f16x3-direct": ("f16x3", "direct", SMALL, 3000),
    "f16x3-wino26": ("f16x3", "wino26", SMALL, 3000),
}
_CASES = [(c, api) for c in ("f16x3", "fp32", "f16", "f16x3-128x192") for api in soak.APIS]
_CASES += [("f16x3-direct", "feedin_one_element"), ("f16x3-wino26", "feed_overlapped")]
if LONG:
    _CONFIGS["long-128x192"] = ("f16x3", "auto", LARGE, 20000)
    _CONFIGS["long-540x960"] = ("f16x3", "auto", (540, 960), 2000)
    _CASES += [(c, api) for c in ("long-128x192", "long-540x960") for api in soak.APIS]
_SHARED = {}


def _config(name):
    """(model, pool, T, sample, expected frames) of a configuration: built once; the expected frames are computed by the first case
    that asks, AFTER its stream (so that no clip disturbs that stream's memory samples), and shared unchanged from then on"""
    if name not in _SHARED:
        precision, wide, size, steady = _CONFIGS[name]
        m = _model(precision, wide_conv=wide)
        T = _frames(m, steady)
        _SHARED[name] = dict(model=m, pool=_pool(size), T=T, sample=soak.sample_indices(T), want=None, got={})
    return _SHARED[name]


def _want(cfg):
    if cfg["want"] is None:
        cfg["want"] = soak.expected_frames(cfg["model"], cfg["pool"], cfg["T"], cfg["sample"])
    return cfg["want"]


def _streamed(name, api):
    """the configuration's stream through ``api``: run once (test a. asserts on it, the oracle anchor reads its last window), with what
    has to be read off the engine while it is this stream's: -> (cfg, (frames, log, (step keys, plans, plans per step), SOAK line))"""
    cfg = _config(name)
    if api not in cfg["got"]:
        m, T = cfg["model"], cfg["T"]
        m.release_stream_buffers()                         # every case starts from no rings, no plans, no graphs
        got, log, seconds = _timed_stream(m, cfg["pool"], api, T, sample=cfg["sample"])
        count = soak.steady_plan_count(m._stream_eng, log, soak.steady_start(m), T)
        cfg["got"][api] = got, log, count, _line("%s %s %dx%d" % (name, api, *_CONFIGS[name][2]), T, seconds, m)
    return cfg, cfg["got"][api]


@pytest.mark.parametrize("name,api", _CASES)
def test_long_stream_matches_its_windows(name, api):
    from bsvd_amd.stream_plan import RING_PERIOD
    cfg, (got, log, (keys, plans, per_step), line) = _streamed(name, api)
    m, T, sample = cfg["model"], cfg["T"], cfg["sample"]
    lo = soak.steady_start(m)
    assert T - lo >= _CONFIGS[name][3] and len(log) == T + m.shift_num + 1
    print(line)
    want = _want(cfg)
    bad = [t for i, t in enumerate(sample) if not torch.equal(got[i], want[i])]
    assert not bad, "%d of %d sampled frames differ from their windows, first at t = %s (max-abs %.3g)" % (
        len(bad), len(sample), bad[:8], float((got - want).abs().max()))
    # checked frames that went in after the fill and came out before the flush: in every ring phase
    assert {t % RING_PERIOD for t in sample if lo <= t < T - m.shift_num - 1} == set(range(RING_PERIOD))
    # steady state, up to the first flush feed: one replay per feed and nothing else moves
    soak.assert_steady(log, lo, T, what=(name, api))
    assert per_step == 2 and keys == RING_PERIOD and plans == RING_PERIOD * per_step, (keys, plans, per_step)
    assert log[T - 1]["graphs"] >= RING_PERIOD and log[T - 1]["graph_evictions"] == 0


# ---- g. one oracle anchor -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f16x3", "fp32"])
def test_last_window_against_the_cpu_oracle(name):
    """the last windowed sample of case a. (36 x 52, 33 frames) against oracle.bsvd_oracle.bsvd_clip on the CPU, within the project's
    1e-3 budget: the soak's comparator is the engine's own clip schedule -- this ties it to the independent restatement once"""
    from oracle import bsvd_oracle as O
    cfg, (got, _, _, _) = _streamed(name, "feedin_one_element")
    m, T, sample = cfg["model"], cfg["T"], cfg["sample"]
    i, t = max((i, t) for i, t in enumerate(sample) if t < T - soak.EDGE)
    lo, hi = soak.window(t, T, m.shift_num)
    assert hi - lo == 2 * m.shift_num + 1
    ref = O.bsvd_clip(cfg["pool"].clip(lo, hi).cpu()[None], O.to_torch_state(_state(17)))[0, t - lo]
    err = float((got[i].cpu() - ref).abs().max())
    print("SOAK oracle anchor %s: frame %d of %d, window [%d, %d): max-abs vs CPU oracle %.3e (budget 1e-3)" % (name, t, T, lo, hi, err))
    assert err < 1e-3


# ---- b. streaming_forward over a long clip --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip500():
    m = _model("f16x3")
    pool, T = _pool(SMALL), 500
    sample = soak.sample_indices(T)
    x = pool.clip(0, T)
    return m, x, sample, soak.expected_frames(m, pool, T, sample)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("chunk", [1, 2, 3, "auto"])
def test_streaming_forward_long_clip(clip500, chunk, overlap):
    m, x, sample, want = clip500
    m.release_stream_buffers()
    m.stream_chunk, m.stream_overlap = chunk, overlap
    n = m._pick_chunk(x.shape[0], x.shape[-2], x.shape[-1])
    assert n == (2 if chunk == "auto" else chunk)
    seen = []
    t0 = time.perf_counter()
    for call in range(3):
        y = m.streaming_forward(x)
        eng = m._stream_engs[n]
        seen.append(dict(eng.stats, plans=len(eng.plans)))
        bad = [t for t in sample if not torch.equal(y[t], want[sample.index(t)])]
        assert not bad, (call, bad[:8])
        del y
    torch.cuda.synchronize()
    print("SOAK streaming_forward chunk %s overlap %s: 3 x %d frames %.2f s, per call %s"
          % (chunk, overlap, x.shape[0], time.perf_counter() - t0, [(s["graph_captures"], s["batch_launches"], s["plans"]) for s in seen]))
    # the second call meets no new key: no batched launch, no plan (it captures what the first met once: fill and flush) ...
    assert seen[1]["batch_launches"] == seen[0]["batch_launches"] and seen[1]["plans"] == seen[0]["plans"]
    # ... and the third adds nothing: no capture, no batched launch, no plan -- every step one replay
    for name in ("graph_captures", "batch_launches", "plans"):
        assert seen[2][name] == seen[1][name], (name, seen)
    assert seen[2]["graph_replays"] - seen[1]["graph_replays"] == seen[2]["steps"] - seen[1]["steps"] - 1     # (the discarded flush step launches nothing)


# ---- c. repeated streams reuse their graphs -------------------------------------------------------------------------------------------
def test_repeated_streams_reuse_their_graphs():
    """Streams of 50 ... 59 frames (every residue of the ring period: ten flush phases), each api, three passes with reset() between:
    pass 2 plans nothing and launches nothing directly, pass 3 adds nothing at all; an abandoned stream in the middle (23 feeds, then
    reset()) changes neither the counts nor the next stream's frames."""
    m, pool = _model("f16x3"), _pool(SMALL)
    lengths = list(range(50, 60))
    want = {T: soak.expected_frames(m, pool, T, soak.sample_indices(T)) for T in lengths}
    t0 = time.perf_counter()
    for api in soak.APIS:
        m.release_stream_buffers()
        counts = []
        for rep in range(3):
            for T in lengths:
                if rep == 2 and T == 55:
                    before = dict(m._stream_eng.stats, plans=len(m._stream_eng.plans), graphs=soak.real_graphs(m._stream_eng))
                    _, log = soak.run_stream(m, pool, api, 80, stop=lambda k: k >= 23, mem=False)
                    assert len(log) == 23
                    after = dict(m._stream_eng.stats, plans=len(m._stream_eng.plans), graphs=soak.real_graphs(m._stream_eng))
                    for name in ("graph_captures", "batch_launches", "plans", "graphs"):
                        assert after[name] == before[name], (api, name)
                got, _ = soak.run_stream(m, pool, api, T, mem=False)
                assert got.shape[0] == T and torch.equal(got, want[T]), (api, rep, T)
            eng = m._stream_eng
            counts.append(dict(eng.stats, plans=len(eng.plans), graphs=soak.real_graphs(eng)))
        assert counts[1]["batch_launches"] == counts[0]["batch_launches"] and counts[1]["plans"] == counts[0]["plans"], (api, counts)
        for name in ("graph_captures", "batch_launches", "plans", "graphs"):
            assert counts[2][name] == counts[1][name], (api, name, counts)
        assert counts[2]["graphs"] == counts[2]["graph_captures"] and counts[2]["graph_evictions"] == 0
        print(_line("repeated streams 50..59 x 3 %s" % api, 3 * sum(lengths) + 23, time.perf_counter() - t0, m))


# ---- d. build / release cycles --------------------------------------------------------------------------------------------------------
def test_build_release_cycles_give_the_memory_back():
    """Ten cycles of: stream 60 frames, then in turn release_stream_buffers() / the other frame size (36 x 52 <-> 52 x 36) / an in-place
    weight update followed by one clip_forward.  After every cycle torch's allocator is back at the first cycle's numbers.

    Two numbers: ``requested_bytes`` (the bytes of the live tensors as they were asked for -- exact, whatever the allocator's history)
    must be the first cycle's ALWAYS; ``memory_allocated`` (the bytes of the blocks handed out for them) as well, except across a
    re-pack: the caching allocator hands out a cached block up to 1 MiB larger than asked without splitting it, so the new pack's blocks
    need not add up to the old pack's (measured: + 1.5 MB on a 52 MB pack).  There it must stay within less than the smaller of the two
    things that could have been kept -- a ring set, a weight pack -- and is taken as the number to hold from then on."""
    m = _model("f16x3")
    sizes = [SMALL, SMALL[::-1]]
    pools = {s: _pool(s) for s in sizes}
    T = 60
    sample = soak.sample_indices(T)
    assert sample == list(range(T))

    def stream(size, api):
        got, _ = soak.run_stream(m, pools[size], api, T, sample, mem=False)
        want = m.clip_forward(pools[size].clip(0, T))
        assert torch.equal(got, want), (size, api)
        return got.cpu()

    def held(collect=True):
        if collect:                                # (reference cycles: a dropped engine or pack must not wait for the collector's own schedule)
            gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["requested_bytes.all.current"], torch.cuda.memory_allocated()

    stream(SMALL, "feedin_one_element")
    ring_bytes = m._stream_eng.ring_bytes
    pack_bytes = sum(t.numel() * t.element_size() for ts in list(m._packed.tensors.values()) + [(w,) for w in m._packed.wino.values()]
                     for t in ts if t is not None)
    m.release_stream_buffers()
    base = held()
    assert ring_bytes > 2 ** 20 and pack_bytes > 2 ** 20
    size, updates = SMALL, 0
    t0 = time.perf_counter()
    for cycle in range(10):
        api = soak.APIS[cycle % 2]
        got = stream(size, api)
        eng = m._stream_eng
        assert eng is not None and held(collect=False)[0] == base[0] + eng.ring_bytes          # the rings are all a built stream holds
        rings, graphs = eng.rings, eng.graphs      # (the engine itself is let go: it holds its executor, and that the weight pack)
        del eng
        if cycle % 3 == 0:
            m.release_stream_buffers()
        elif cycle % 3 == 1:                       # the other frame size: its first feed drops the old rings and graphs and builds new ones
            size = sizes[1 - sizes.index(size)]
            stream(size, api)
            assert not rings and not graphs and m._stream_eng.rings is not rings
            m.release_stream_buffers()
        else:                                      # in-place weight update: the next forward re-packs and drops the engines with the old pack
            with torch.no_grad():
                for p in m.parameters():
                    p.mul_(1.01)
            m.clip_forward(pools[size].clip(0, 1))
            assert m._stream_eng is None and not rings and not graphs
            req, alloc = held()
            assert req == base[0], (cycle, "after the re-pack", req, base)
            assert abs(alloc - base[1]) < min(ring_bytes, pack_bytes), (cycle, "after the re-pack", alloc, base, ring_bytes, pack_bytes)
            base = (req, alloc)
            new = stream(size, api)                # == the NEW weights' clip_forward (asserted in stream) ...
            assert not torch.equal(new, got)       # ... and not what the old weights gave: no stale graph, no stale pack
            updates += 1
            m.release_stream_buffers()
        assert m._stream_eng is None and not m._stream_engs
        now = held()
        assert now == base, (cycle, now, base)
    assert updates == 3
    print("SOAK build/release: 10 cycles (release / frame-size switch / weight update) %.2f s, requested %d B, memory_allocated %d B after "
          "every cycle (rings %d B, pack %d B)" % (time.perf_counter() - t0, base[0], base[1], ring_bytes, pack_bytes))


# ---- e. LiveStream --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,overlap_blocks", [(2, None), (3, False)])
def test_live_stream_long_feed(depth, overlap_blocks):
    from bsvd_amd.frame_io import frames_to_input, output_to_frames
    from bsvd_amd.pipeline import LiveStream
    m = _model("f16x3")
    H, W = SMALL
    sigma = 30.0 / 255.0
    T = _frames(m, 500)
    u8 = np.random.RandomState(11).randint(0, 256, size=(soak.POOL, H, W, 3), dtype=np.uint8)
    pool = soak.Pool.of(frames_to_input(torch.from_numpy(u8).to(_dev()), sigma))
    want = output_to_frames(soak.expected_all(m, pool, T)).cpu().numpy()
    assert want.shape == (T, H, W, 3)
    live = LiveStream(m, sigma=sigma, depth=depth, overlap_blocks=overlap_blocks, frame_shape=(H, W))
    assert live.latency_final and live.overlap == (overlap_blocks is None)
    lat = live.latency
    assert lat == m.shift_num + depth - 1 + (1 if live.overlap else 0)
    gc.collect()                               # (the allocator's numbers are the process's: earlier garbage goes before the feed, not during)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_out, bad, mem = 0, [], []
    for k in range(T):
        y = live.feed(u8[k % soak.POOL])
        assert (y is not None) == (k >= lat), k
        if y is not None:
            if not np.array_equal(y, want[k - lat]):       # the frame fed ``latency`` feeds earlier
                bad.append(k - lat)
            n_out += 1
        del y
        mem.append((torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
    for y in live.flush():
        if not np.array_equal(y, want[n_out]):
            bad.append(n_out)
        n_out += 1
    seconds = time.perf_counter() - t0
    assert n_out == T and not bad, (n_out, T, bad[:8])
    lo = soak.steady_start(m) + depth + 1
    assert all(a == mem[lo][0] for a, _ in mem[lo:]), ("memory_allocated", sorted({a for a, _ in mem[lo:]}))
    assert all(r <= mem[lo][1] for _, r in mem[lo:])
    print(_line("LiveStream rgb24 depth %d overlap %s" % (depth, live.overlap), T, seconds, m))


# ---- f. two host threads, two models --------------------------------------------------------------------------------------------------
def _two_threads(models, pool, apis, T, sample):
    """models[i] through apis[i] on a thread and a HIP stream of its own, barrier start; -> the two threads' sampled frames.  An
    exception in a thread stops the other one and is re-raised here; the joins carry a timeout; nothing is retried."""
    start, stop = threading.Barrier(2), threading.Event()
    streams = [torch.cuda.Stream(_dev()) for _ in models]
    got, errors = {}, []

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                start.wait(timeout=60)
                out, log = soak.run_stream(models[i], pool, apis[i], T, sample, stop=lambda k: stop.is_set(), mem=False)
                streams[i].synchronize()
                assert len(log) == T + models[i].shift_num + 1, "stopped by the other thread's failure"
                got[i] = out
        except BaseException as e:             # noqa: B036 -- collected, re-raised in the main thread
            errors.append(e)
            stop.set()
            start.abort()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(models))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    if errors:
        raise errors[0]
    torch.cuda.synchronize()
    return got


def test_two_host_threads_two_models():
    """header: "calls on distinct streams may run concurrently".  Two models with different weights, two Python threads, a HIP stream
    each, one on feedin_one_element, the other on feed_overlapped, then swapped: each thread's frames equal its model's solo run."""
    models = [_model("f16x3", seed=17), _model("f16x3", seed=18)]
    pool = _pool(SMALL)
    T = _frames(models[0], 300)
    sample = soak.sample_indices(T)
    solo = {(i, api): soak.run_stream(m, pool, api, T, sample, mem=False)[0] for i, m in enumerate(models) for api in soak.APIS}
    assert not torch.equal(solo[0, soak.APIS[0]], solo[1, soak.APIS[0]])
    for i in range(2):
        assert torch.equal(solo[i, soak.APIS[0]], solo[i, soak.APIS[1]])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for apis in (soak.APIS, soak.APIS[::-1]):
        got = _two_threads(models, pool, apis, T, sample)
        for i in range(2):
            bad = [t for j, t in enumerate(sample) if not torch.equal(got[i][j], solo[i, apis[i]][j])]
            assert not bad, "thread %d (%s): %d of %d sampled frames differ from the model's solo run, first at t = %s" % (
                i, apis[i], len(bad), len(sample), bad[:8])
    print("SOAK two host threads x two models, apis swapped: 4 x %d frames %.2f s" % (T, time.perf_counter() - t0))


# ---- graph eviction -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("api", soak.APIS)
def test_graph_eviction_keeps_streaming(api):
    """``max_graphs`` just above one ring period's working set: every stream's fill and flush keys push the steady-state graphs out, the
    next stream captures them again -- after a device drain, never under a running replay.  Frames still equal their windows, the table
    stays within its limit, captures keep growing; plans, live graphs and device memory do not."""
    from bsvd_amd.stream_plan import RING_PERIOD
    m, pool, T = _model("f16x3"), _pool(SMALL), 200
    sample = soak.sample_indices(T)
    want = soak.expected_frames(m, pool, T, sample)
    got, log = soak.run_stream(m, pool, api, T, sample)
    assert torch.equal(got, want)
    eng = m._stream_eng
    working_set, _, _ = soak.steady_plan_count(eng, log, soak.steady_start(m), T)
    assert working_set == RING_PERIOD and eng.stats["graph_evictions"] == 0
    eng.max_graphs = working_set + 1
    eng._evict()                                           # down to the limit before the streams below
    rows = []
    t0 = time.perf_counter()
    for rep in range(4):
        got, log = soak.run_stream(m, pool, api, T, sample)
        assert m._stream_eng is eng and torch.equal(got, want), rep
        assert len(eng.graphs) <= eng.max_graphs
        soak.assert_steady(log, soak.steady_start(m), T, what=("eviction", api, rep))
        rows.append(dict(log[-1], table=len(eng.graphs)))
    torch.cuda.synchronize()
    for a, b in zip(rows[1:], rows[2:]):
        assert b["graph_captures"] - a["graph_captures"] == RING_PERIOD            # the steady state, captured again by every stream
        assert b["graph_evictions"] - a["graph_evictions"] == RING_PERIOD          # ... after the flush keys pushed it out
        assert b["plans"] == a["plans"] and b["graphs"] <= eng.max_graphs and b["allocated"] == a["allocated"] and b["reserved"] <= a["reserved"]
    print(_line("eviction max_graphs %d %s x 4" % (eng.max_graphs, api), 4 * T, time.perf_counter() - t0, m,
                "  evictions %d" % eng.stats["graph_evictions"]))
