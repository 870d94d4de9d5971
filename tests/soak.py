"""Long-stream soak helpers (not a conftest): a stream of any length is checked against SHORT clips.

The network has ``shift_num`` temporal-fusion layers in sequence, each reaching one frame either way, so output frame t depends on input
frames t - shift_num ... t + shift_num and on nothing else: ``clip_forward(x[t - r : t + r + 1])[r]`` with r = shift_num IS frame t of any
longer stream, bit for bit within a precision mode (every schedule is bit-identical per output; the zero halos at the window's ends only
reach layer outputs outside frame t's cone).  Near the stream's ends the window is cut -- the stream's own ends are zeros too.  Neither a
reference run of the whole stream nor memory for it is needed (tests/test_soak_cpu.py checks the premise and that radius r - 1 fails).

The input is a pool of POOL = 97 distinct frames, frame t of the stream being pool[t % 97]: 97 is prime, hence coprime to the ring period
(10) -- every ring phase meets every pool frame, and a slot that is stale by 10, 20, ... steps holds a different frame and shows in the
VALUES.  No case holds its whole input.
"""
import gc

import numpy as np
import torch

POOL = 97          # prime: coprime to stream_plan.RING_PERIOD
RESIDUE = 13       # sampled: every t with t % POOL == RESIDUE ...
EDGE = 40          # ... and the first and the last EDGE frames (pipeline fill and flush)

APIS = ("feedin_one_element", "feed_overlapped")


class Pool:
    """POOL seeded random frames [POOL, C, H, W] in [0, 1) on ``device``; ``frame(t)`` is a VIEW (no allocation per step)"""

    def __init__(self, C, H, W, seed, device="cpu", sigma=None):
        rs = np.random.RandomState(seed)
        x = rs.random_sample((POOL, C, H, W)).astype(np.float32)
        if sigma is not None:                # the last channel as the constant noise map a caller appends
            x[:, -1] = np.float32(sigma)
        self.frames = torch.from_numpy(x).to(device)

    @classmethod
    def of(cls, frames):
        self = cls.__new__(cls)
        assert frames.shape[0] == POOL
        self.frames = frames
        return self

    def frame(self, t):
        return self.frames[t % POOL][None]

    def clip(self, lo, hi):
        """frames lo ... hi - 1 of the stream as one tensor (a short clip: a window or an end block)"""
        return self.frames[torch.arange(lo, hi, device=self.frames.device) % POOL]


def sample_indices(T, edge=EDGE):
    """the stream positions whose output frames are kept and checked, ascending"""
    return sorted({t for t in range(T) if t % POOL == RESIDUE or t < edge or t >= T - edge})


def window(t, T, radius):
    """[lo, hi): the input frames output frame t of a T-frame stream depends on"""
    return max(0, t - radius), min(T, t + radius + 1)


def _clip(model, pool, lo, hi):
    return model.clip_forward(pool.clip(lo, hi))


def expect(model, pool, t, T, radius=None, clip=_clip):
    """frame t of the T-frame stream, from the clip schedule over its window"""
    lo, hi = window(t, T, model.shift_num if radius is None else radius)
    return clip(model, pool, lo, hi)[t - lo]


def expected_frames(model, pool, T, sample, radius=None, clip=_clip, edge=EDGE):
    """[len(sample), out_ch, H, W]: every sampled frame from the clip schedule.  The two end blocks take ONE clip each -- the first
    ``edge`` frames are ``clip(x[0 : edge + r])[:edge]`` (frame t needs the frames up to t + r), the last ``edge`` the mirror image --
    the frames between them one window each."""
    r = model.shift_num if radius is None else radius
    head_hi, tail_lo = min(T, edge + r), max(0, T - edge - r)
    head = tail = None
    out = []
    for t in sample:
        if t < edge:
            head = clip(model, pool, 0, head_hi) if head is None else head
            out.append(head[t])
        elif t >= T - edge:
            tail = clip(model, pool, tail_lo, T) if tail is None else tail
            out.append(tail[t - tail_lo])
        else:
            out.append(expect(model, pool, t, T, r, clip))
    return torch.stack(out)


def expected_all(model, pool, T, block=64, clip=_clip):
    """[T, out_ch, H, W]: EVERY frame of the stream from the clip schedule, in blocks: ``clip(x[a - r : b + r])[r : -r]`` is frames
    a ... b - 1 (each has its whole window inside the clip, or the clip ends where the stream ends) -- about (block + 2 r) / block of
    the work of one pass over the stream, never more than block + 2 r frames at a time."""
    r = model.shift_num
    out = []
    for a in range(0, T, block):
        b = min(T, a + block)
        lo, hi = max(0, a - r), min(T, b + r)
        out.append(clip(model, pool, lo, hi)[a - lo:b - lo])
    return torch.cat(out)


def flush_feeds(model, api):
    """(None feeds after the last frame, whether a ``last=True`` call follows them)"""
    return model.shift_num + 1, api == "feed_overlapped"


def latency(model, api):
    return model.shift_num + (1 if api == "feed_overlapped" else 0)


def real_graphs(eng):
    return sum(1 for g in eng.graphs.values() if g[0] is not None)


def _snapshot(eng, mem):
    row = dict(eng.stats, plans=len(eng.plans), graphs=real_graphs(eng), key=next(reversed(eng.graphs)) if eng.graphs else None)
    if mem:
        row["allocated"], row["reserved"] = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    return row


def run_stream(model, pool, api, T, sample=None, stop=None, mem=True):
    """Feeds the T-frame stream through ``api`` with its flush protocol (shift_num + 1 feeds of None; ``feed_overlapped``: then the
    ``last=True`` call) and ``reset()``.  The sampled output frames go into ONE preallocated buffer, so the loop's live allocations
    do not change from step to step.  ``stop(k)``: asked before feed k; True abandons the stream there (then ``reset()``).
    -> (frames [len(sample), out_ch, H, W], log): one log row per feed -- the engine's stats, ``plans``, ``graphs`` (captured ones),
    ``key`` (the step's entry in ``eng.graphs``), ``allocated`` / ``reserved`` (torch's allocator, with ``mem``).  The allocator's
    numbers are the whole process's: with ``mem`` the garbage of whatever ran before (models in reference cycles) is collected first,
    so that Python's collector cannot hand back ITS device memory in the middle of this stream."""
    if mem:
        gc.collect()
    sample = sample_indices(T) if sample is None else list(sample)
    where = {t: i for i, t in enumerate(sample)}
    feed = getattr(model, api)
    lat = latency(model, api)
    nflush, last_call = flush_feeds(model, api)
    x0 = pool.frame(0)
    out = torch.empty((len(sample), model.net.out_ch) + tuple(x0.shape[-2:]), dtype=torch.float32, device=x0.device)
    log, n_out = [], 0
    for k in range(T + nflush):
        if stop is not None and stop(k):
            break
        y = feed(pool.frame(k) if k < T else None)
        assert (y is not None) == (lat <= k < T + lat), (api, k, T)
        if y is not None:
            if n_out in where:
                out[where[n_out]].copy_(y[0])
            n_out += 1
        del y
        log.append(_snapshot(model._stream_eng, mem))
    else:
        if last_call:
            assert feed(None, last=True) is None
        assert n_out == T, (n_out, T)
    model.reset()
    return out, log


def steady_start(model):
    """first step of the region every plan of which is a replayed graph: the pipeline fill (shift_num steps, one more for the lagged
    schedule -- rounded up to 2 * shift_num) plus two sightings of each of the RING_PERIOD phases (the second one captures)"""
    from bsvd_amd.stream_plan import RING_PERIOD
    return 2 * model.shift_num + 2 * RING_PERIOD


def assert_steady(log, lo, hi, what=""):
    """rows lo ... hi - 1 of a run_stream log: nothing is captured, planned or launched layer by layer, every feed is exactly one
    graph replay, torch's allocator holds the same number of bytes at every step and reserves no more"""
    from bsvd_amd.stream_plan import RING_PERIOD
    assert hi - lo >= 2 * RING_PERIOD, (lo, hi)
    a = log[lo]
    for k in range(lo + 1, hi):
        b = log[k]
        for name in ("graph_captures", "batch_launches", "plans", "graphs"):
            assert b[name] == a[name], (what, name, k, a[name], b[name])
        assert b["graph_replays"] == a["graph_replays"] + (k - lo), (what, k, a["graph_replays"], b["graph_replays"])
        assert b["steps"] == a["steps"] + (k - lo), (what, k)
        if "allocated" in a:
            assert b["allocated"] == a["allocated"], (what, "memory_allocated", k, a["allocated"], b["allocated"])
            assert b["reserved"] <= a["reserved"], (what, "memory_reserved", k, a["reserved"], b["reserved"])


def steady_plan_count(eng, log, lo, hi):
    """(distinct step keys, distinct plans among them, plans per step) over rows lo ... hi - 1, read off the engine's own tables"""
    keys = {row["key"] for row in log[lo:hi]}
    per_step = {len([s for s in key if s != "lag"]) for key in keys}
    assert len(per_step) == 1, per_step
    sigs = {s for key in keys for s in key if s != "lag"}
    assert all(s in eng.plans for s in sigs)
    return len(keys), len(sigs), per_step.pop()
