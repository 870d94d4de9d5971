"""The table of cross-stream hand-overs (tests/stream_hold.py: EDGES) names exactly the ordering calls of bsvd_amd/pipeline.py, so a
hand-over added without a held test fails here; ``without`` puts back what it took; the C clip of tests/test_gpu_stream_order.py holds one
cut for the detector's model."""
import os

import numpy as np
import pytest

import scene_model as M
import stream_hold as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sites():
    with open(os.path.join(ROOT, "bsvd_amd", "pipeline.py")) as f:
        return SH.order_sites(f.read())


def test_the_edge_table_names_exactly_the_ordering_calls_of_the_pipelines():
    sites = _sites()
    table = sorted(((c, f, call) for c, f, call, *_ in SH.EDGES), key=repr)
    assert len(sites) >= 20 and all(c in ("_Ticket", "ClipPipeline", "LiveStream") for c, _, _ in sites)
    missing = [s for s in sites if s not in table]
    stale = [s for s in table if s not in sites]
    assert not missing, "hand-overs of pipeline.py without a row (and a held test) in stream_hold.EDGES: %r" % (missing,)
    assert not stale, "rows of stream_hold.EDGES that pipeline.py no longer has: %r" % (stale,)
    assert table == sites                                    # the same call twice in one method needs two rows


def test_every_row_names_a_test_of_the_gpu_file_and_every_wait_a_mutant():
    with open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")) as f:
        gpu = f.read()
    for c, fn, call, producer, consumer, test, mutant in SH.EDGES:
        assert {producer, consumer} <= {"host", "up", "comp", "down"} and producer != consumer
        assert "def %s(" % test.split("[")[0] in gpu, (call, test)
        for m in (mutant or "").split(", "):
            if m:
                assert "def %s(" % m.split()[1].split("[")[0] in gpu, (call, m)
        waits = any(call.endswith(e) or (".%s(" % e) in call for e in ("wait_event", "wait_stream", "synchronize"))
        assert bool(mutant) == waits, "%s.%s: %s -- every wait has a mutant, nothing else has" % (c, fn, call)


def test_the_walk_sees_a_hand_over_that_is_added():
    src = ("import torch\nclass P:\n    def go(self, s, e, t):\n        with torch.cuda.stream(s):\n            e.record()\n"
           "        s.wait_stream(self.other)\n        t.record_stream(s)\n        e.synchronize()\n        s.wait_event(e)\n"
           "def free(e):\n    e.record()\n")
    assert SH.order_sites(src) == sorted([("P", "go", "torch.cuda.stream(s)"), ("P", "go", "e.record()"), ("P", "go", "s.wait_stream(self.other)"),
                                          ("P", "go", "t.record_stream(s)"), ("P", "go", "e.synchronize()"), ("P", "go", "s.wait_event(e)"),
                                          (None, "free", "e.record()")], key=repr)


class _Obj:
    def wait(self, x):
        return ("waited", x)


def test_without_removes_one_method_and_puts_it_back():
    a, b = _Obj(), _Obj()
    with SH.without(a, "wait") as got:
        assert got is a and a.wait(1) is None and b.wait(1) == ("waited", 1)
    assert a.wait(2) == ("waited", 2) and "wait" not in a.__dict__
    with pytest.raises(KeyError):
        with SH.without(a, "wait"):
            assert a.wait(3) is None
            raise KeyError("inside")
    assert a.wait(4) == ("waited", 4) and "wait" not in a.__dict__
    a.wait = lambda x: ("own", x)                          # an attribute of the instance comes back as it was
    with SH.without(a, "wait"):
        assert a.wait(5) is None
    assert a.wait(6) == ("own", 6)
    with pytest.raises(AttributeError):
        with SH.without(a, "no_such_method"):
            pass


def test_the_two_scene_clip_holds_exactly_one_cut():
    """configuration C: 23 frames of 30 x 42 (the top-left of the margin clip at 32 x 48), scenes of 12 and 11 frames: the model alone
    scores exactly one cut at the default threshold, far from it on both sides"""
    G = SH
    x, starts = G.two_scene_clip()
    assert x.shape == (sum(G.C_LENGTHS), 4) + G.C_SIZE and starts == [0, G.C_LENGTHS[0]]
    found, scores = M.cuts(x, picture=G.C_SIZE)
    assert found == starts[1:]
    assert scores[starts[1]] >= 20.0 and max(s for t, s in enumerate(scores) if t != starts[1]) <= 5.0
    assert len({x[t].tobytes() for t in range(len(x))}) == len(x)                 # every frame differs
    assert np.array_equal(M.cuts(x[:6], picture=G.C_SIZE)[0], [])                 # the short second stream: one scene
