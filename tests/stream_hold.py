"""Test infrastructure for stream-order tests: a bounded delay (a "hold") on one HIP stream, so that a consumer that is not ordered behind
its producer reads old bytes on demand; a probe that tells whether two streams can run side by side at all; ``without`` -- one wait
removed, the mutants that show the tests bite --; and EDGES, the table of every cross-stream hand-over of bsvd_amd/pipeline.py.

A hold is ``torch.cuda._sleep(cycles)``: one thread of one workgroup counting a clock down.  The trip count is the bound; it reads no
memory and waits for nothing, and it takes no CU away from what runs beside it.  The clock's rate is not assumed: ``calibrate`` measures
cycles per millisecond once per process, from device events around two holds of different lengths (the slope, so that the launch does
not count).

HIP gives a process a limited number of hardware queues and lets streams share them.  Two streams on one queue run in order whatever the
code does, and no ordering test can bite on them: every held test asserts ``overlaps(producer, consumer)`` on the pipeline's own stream
objects first (``on_distinct_queues``), builds the pipeline again -- keeping the earlier streams alive as spares -- until they do, and
fails with the pair named if that cannot be reached."""
import ast
import contextlib
import time

import torch

HOLD_MS = 3.0               # the starting length: two orders above a launch; raised to 10 x the unheld step where that is longer
_CAL = {}
_ONE = {}
SPARE = []                  # streams kept alive so that later ones land on other queues
NOTES = []                  # what the probes measured, one line each (printed as they are made: run pytest with -s to see them)


def note(line):
    NOTES.append(line)
    print("stream-order: " + line, flush=True)


def calibrate(device=None):
    """cycles of ``torch.cuda._sleep`` per millisecond on ``device``: the slope between two holds, the median of three readings"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev not in _CAL:
        c1, c2 = 2_000_000, 10_000_000
        with torch.cuda.device(dev):
            s = torch.cuda.Stream()
            slopes = []
            with torch.cuda.stream(s):
                torch.cuda._sleep(c1)                 # the first launch loads the kernel
                s.synchronize()
                for _ in range(3):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()
                    torch.cuda._sleep(c1)
                    ev[1].record()
                    torch.cuda._sleep(c2)
                    ev[2].record()
                    s.synchronize()
                    t1, t2 = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
                    slopes.append((c2 - c1) / (t2 - t1))
            SPARE.append(s)
        slopes.sort()
        if not (slopes[1] > 0 and slopes[2] <= 1.5 * slopes[0]):
            raise RuntimeError("calibrate: the hold's length does not follow its cycle count: %r cycles / ms" % (slopes,))
        _CAL[dev] = slopes[1]
        note("calibrate: %.0f cycles / ms (three slopes %s)" % (slopes[1], ", ".join("%.0f" % v for v in slopes)))
    return _CAL[dev]


def hold(stream, ms=None):
    """one bounded delay of ``ms`` milliseconds on ``stream`` (one thread; returns at once)"""
    ms = HOLD_MS if ms is None else ms
    cycles = int(calibrate(stream.device) * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def overlaps(a, b, ms=4.0):
    """True if a 1-element kernel on ``b``, enqueued behind a hold on ``a``, completes while the hold is still running -- by the host's
    ``event.query()`` and by the device's event times, both.  False: the two streams share a hardware queue (or the device runs one
    kernel at a time), and no ordering test between them can bite."""
    if a.device not in _ONE:
        _ONE[a.device] = torch.zeros(1, device=a.device)
    one = _ONE[a.device]
    torch.cuda.synchronize(a.device)
    t0, a_end, b_end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    t0.record(a)
    hold(a, ms)
    a_end.record(a)
    with torch.cuda.stream(b):
        one.add_(1.0)
        b_end.record()
    deadline = time.perf_counter() + 4 * ms / 1e3
    seen = False
    while time.perf_counter() < deadline and not a_end.query():
        if b_end.query():
            seen = not a_end.query()
            break
    torch.cuda.synchronize(a.device)
    by_time = t0.elapsed_time(b_end) < t0.elapsed_time(a_end) - 0.25 * ms
    return bool(seen and by_time)


def on_distinct_queues(make, pairs, what, tries=12):
    """``make()`` -> an object with stream attributes; ``pairs``: (producer attribute, consumer attribute).  Builds the object until every
    pair overlaps, keeping the streams of the earlier ones alive as spares.  -> (object, number of rebuilds).  Fails, naming the pairs,
    if ``tries`` objects did not get there."""
    import pytest
    bad = []
    for n in range(tries):
        obj = make()
        bad = [(p, c) for p, c in pairs if not overlaps(getattr(obj, p), getattr(obj, c))]
        if not bad:
            if n:
                note("%s: %d rebuild(s) until %s ran side by side" % (what, n, pairs))
            return obj, n
        SPARE.extend(getattr(obj, name) for name in {x for pc in pairs for x in pc})
    pytest.fail("%s: after %d rebuilds the streams %s still share a hardware queue: no ordering test can bite" % (what, tries, bad))


@contextlib.contextmanager
def without(obj, method):
    """``obj.method`` is a no-op inside the block: one wait removed.  The attribute is set on the instance and taken off again, also when
    the block raises."""
    had = method in getattr(obj, "__dict__", {})
    old = obj.__dict__[method] if had else None
    getattr(obj, method)                                   # a wrong name fails here
    setattr(obj, method, lambda *a, **k: None)
    try:
        yield obj
    finally:
        if had:
            setattr(obj, method, old)
        else:
            delattr(obj, method)


# ---- the hand-overs of bsvd_amd/pipeline.py ---------------------------------------------------------------------------------------------
# One row per call that orders streams, or streams and the host: (class, method, call as written, producer, consumer, held test, mutant).
# tests/test_stream_order_cpu.py walks pipeline.py and asserts that these are exactly its call sites: a hand-over added later fails the
# CPU suite until it has a row, and with it a held test.  ``mutant`` None: the call is a producer's side (an event recorded, a stream
# entered) -- it is covered through the wait that reads it -- or is left alone for the reason given.
LIVE, CLIP = "test_live_stream_under_holds", "test_clip_pipeline_under_holds"
EDGES = [
    ("_Ticket", "finish", "self.slot.downloaded.synchronize()", "down", "host", CLIP, "4c test_mutant_host_reads_before_the_download[clip]"),
    ("ClipPipeline", "submit", "torch.cuda.stream(self.up)", "host", "up", CLIP, None),
    ("ClipPipeline", "submit", "slot.uploaded.record()", "up", "comp", CLIP, None),
    ("ClipPipeline", "submit", "torch.cuda.stream(self.comp)", "host", "comp", CLIP, None),
    ("ClipPipeline", "submit", "self.comp.wait_event(slot.uploaded)", "up", "comp", CLIP, "4a test_mutant_compute_does_not_wait_for_the_upload[clip]"),
    ("ClipPipeline", "submit", "slot.computed.record()", "comp", "down", CLIP, None),
    ("ClipPipeline", "submit", "torch.cuda.stream(self.down)", "host", "down", CLIP, None),
    ("ClipPipeline", "submit", "self.down.wait_event(slot.computed)", "comp", "down", CLIP, "4b test_mutant_download_does_not_wait_for_the_compute[clip]"),
    ("ClipPipeline", "submit", "slot.downloaded.record()", "down", "host", CLIP, None),
    # not mutated: what a missing record_stream does depends on when the allocator hands the block out again; covered from the other
    # side by test_record_stream_holds_under_an_allocation_burst
    ("LiveStream", "_detect", "x.record_stream(self.comp)", "up", "comp", "test_record_stream_holds_under_an_allocation_burst", None),
    ("LiveStream", "_detect", "self._scored.record()", "up", "host", LIVE + "[C]", None),
    ("LiveStream", "_detect", "slot.uploaded.record()", "up", "comp", LIVE + "[C]", None),
    ("LiveStream", "_detect", "self._scored.synchronize()", "up", "host", LIVE + "[C]", "4d test_mutant_host_decides_before_the_score"),
    ("LiveStream", "_pop", "slot.downloaded.synchronize()", "down", "host", LIVE,
     "4c test_mutant_host_reads_before_the_download[live], 4e test_mutant_host_reads_sigma_before_the_download"),
    ("LiveStream", "_step", "torch.cuda.stream(self.up)", "host", "up", LIVE, None),
    ("LiveStream", "_step", "slot.uploaded.record()", "up", "comp", LIVE, None),
    ("LiveStream", "_step", "torch.cuda.stream(self.comp)", "host", "comp", LIVE, None),
    ("LiveStream", "_step", "self.comp.wait_event(slot.uploaded)", "up", "comp", LIVE, "4a test_mutant_compute_does_not_wait_for_the_upload[live]"),
    ("LiveStream", "_step", "slot.computed.record()", "comp", "down", LIVE, None),
    ("LiveStream", "_step", "torch.cuda.stream(self.down)", "host", "down", LIVE, None),
    ("LiveStream", "_step", "self.down.wait_event(slot.computed)", "comp", "down", LIVE, "4b test_mutant_download_does_not_wait_for_the_compute[live]"),
    ("LiveStream", "_step", "slot.downloaded.record()", "down", "host", LIVE, None),
]

ORDER_CALLS = ("wait_event", "wait_stream", "synchronize", "record_stream", "record")


def order_sites(source):
    """every call of ORDER_CALLS and every ``with torch.cuda.stream(...)`` item in ``source`` -> sorted [(class, function, call as written)]"""
    sites = []

    def walk(node, cls, fn):
        for child in ast.iter_child_nodes(node):
            c, f = cls, fn
            if isinstance(child, ast.ClassDef):
                c, f = child.name, None
            elif isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                f = child.name
            elif isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                text = ast.unparse(child)
                if child.func.attr in ORDER_CALLS or ast.unparse(child.func) == "torch.cuda.stream":
                    sites.append((cls, fn, text))
            walk(child, c, f)

    walk(ast.parse(source), None, None)
    return sorted(sites, key=repr)


# ---- the clip of the configuration with cuts='auto' ---------------------------------------------------------------------------------------
C_SIZE = (30, 42)               # a picture that is no multiple of 4 (pad='reflect' -> 32 x 44); one row of two 16 x 16 detector blocks
C_LENGTHS = (12, 11)            # two scenes: latency + depth + 3 = 23 frames at depth 2 with the lagged schedule
C_SEED = 5


def two_scene_clip():
    """the margin clip of tests/scene_model.py in two scenes, its top-left 30 x 42 -> ([T,4,30,42] fp32, starts).  Needs no device."""
    import scene_model
    x, starts = scene_model.margin_clip(32, 48, lengths=C_LENGTHS, seed=C_SEED)
    return x[:, :, :C_SIZE[0], :C_SIZE[1]].copy(), starts
