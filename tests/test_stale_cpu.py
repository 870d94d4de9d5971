"""tests/stale.py without a GPU: the torch.empty wrapper fills what it should and puts the originals back, and the comparison the GPU schedule
tests make -- the same run under fill 0x00 and under fill 0xFF, bit for bit -- catches the three host faults it is there for, on the oracle-backed
executor and the stream engine of tests/test_stream_plan_cpu.py: a ring slot read one step early, a producer that leaves its pad channels
unwritten, a halo buffer consumed before its receive completes.  The unmutated code passes the same comparison."""
import collections

import numpy as np
import pytest
import torch

import stale
from helpers import bsvd_keys
from oracle_exec import OracleExecutor
from seeded import seeded_clip, seeded_state
from test_stream_plan_cpu import _run_feed, _run_lagged, _run_pipeline
from bsvd_amd.netspec import make_netspec
from bsvd_amd.stream_plan import StreamEngine, _Recorder

EVERYWHERE = lambda t: True          # noqa: E731  (the default poisons device and pinned memory only: there is none here)


# ------------------------------------------------------------------------------------------------ the wrapper

def test_wrapper_fills_every_byte_and_restores_the_originals(monkeypatch):
    names = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))
    before = [getattr(o, n) for o, n in names]
    in_dict = "new_empty" in torch.Tensor.__dict__
    for fill in (0xFF, 0x00, 0x5A):
        with stale.poisoned_empty(monkeypatch, fill, where=EVERYWHERE):
            assert all(getattr(o, n) is not b for (o, n), b in zip(names, before))
            a = torch.empty(3, 5)
            made = [a, torch.empty((2, 7), dtype=torch.float16), torch.empty_like(a), torch.empty_like(a, dtype=torch.int64),
                    torch.empty_strided((2, 3), (8, 2)), a.new_empty((4, 2)), a.new_empty(6, dtype=torch.int32), torch.empty(0),
                    torch.empty(5, dtype=torch.uint8)]
            for t in made:
                raw = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes(),), (1,))
                assert bool((raw == fill).all()), (fill, t.shape, t.dtype)
            assert made[4].untyped_storage().nbytes() >= 4 * (8 + 2 * 2 + 1)          # the strided one: the bytes between its elements too
            if fill == 0xFF:
                assert bool(torch.isnan(a).all()) and bool(torch.isnan(made[1]).all()) and bool((made[6] == -1).all())
        assert all(getattr(o, n) is b for (o, n), b in zip(names, before))
        assert ("new_empty" in torch.Tensor.__dict__) == in_dict


def test_wrapper_restores_after_an_exception_and_leaves_unpinned_host_memory_alone(monkeypatch):
    before = torch.empty
    filled = []
    monkeypatch.setattr(stale, "fill_bytes", lambda t, fill: filled.append(t))
    with pytest.raises(RuntimeError, match="inside"):
        with stale.poisoned_empty(monkeypatch, 0xFF):          # the default: device and pinned host memory
            torch.empty(4)
            torch.empty_like(torch.zeros(3))
            raise RuntimeError("inside")
    assert torch.empty is before and not filled


# ------------------------------------------------------------------------------------------------ the comparison and its three mutants

class _DeviceLike(OracleExecutor):
    """The oracle executor reading its input the way the kernels do: the pad channels of an NHWC tensor take part in the dot product, with the
    pack's zero weights (0 * NaN is NaN; the oracle itself slices them away).  What it writes goes through _store."""

    def conv(self, sp, x, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, x_planar=False, y_planar=None, out=None):
        if out is not None:
            y = self.conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar)
            self._store(sp, out, y, y_planar)
            return out
        if x_planar or sp.cin_pad == sp.cin:
            return super().conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar)
        real = x.clone()
        real[..., sp.cin:] = 0
        y = super().conv(sp, real, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar)
        return y + (x[..., sp.cin:] * 0.0).sum()

    def _store(self, sp, out, y, y_planar):
        out.copy_(y)


class _PadsUnwritten(_DeviceLike):
    """mutant: a producer that writes its real channels only"""

    def _store(self, sp, out, y, y_planar):
        if y_planar is None:
            out[..., :sp.out_channels].copy_(y[..., :sp.out_channels])
        else:
            out.copy_(y)


class _EarlyRecorder(_Recorder):
    """mutant: the readers of one layer are handed the ring slot its NEXT production will write"""

    def __init__(self, eng, key):
        super().__init__(eng)
        self.key = key

    def conv(self, sp, x, *a, **kw):
        o = super().conv(sp, x, *a, **kw)
        if sp.key != self.key:
            return o
        ring = self.eng.rings[sp.key]
        assert len(ring) > 1
        nxt = ring[self.count[sp.key] % len(ring)]
        return nxt if nxt.shape[0] == o.shape[0] else nxt[:o.shape[0]]


def _read_early(eng):
    eng.r1 = _EarlyRecorder(eng, eng.net.temp1["down0"].key)


NETS = {"c16": ([16, 32, 64], 16, 16), "pad channels": ([16, 32, 64], 16, 30)}          # chns, mid_ch, interm_ch (30: two pad channels)


def _case(name, T=7):
    chns, mid, interm = NETS[name]
    net = make_netspec(chns, mid, 4, 3, "relu6", interm)
    st = seeded_state(bsvd_keys(chns, mid, 4, 3, interm), 5)
    x = torch.from_numpy(seeded_clip((1, T, 4, 8, 12), 6, kind="sigma30"))[0]
    return net, st, x


def _stream(monkeypatch, fill, net, st, x, ex_cls=_DeviceLike, mutate=None, run=_run_feed):
    """a fresh engine -- rings from torch.empty -- and one clip, everything inside the poisoned context"""
    with stale.poisoned_empty(monkeypatch, fill, where=EVERYWHERE):
        eng = StreamEngine(net, ex_cls(st), 8, 12, 4, alloc=lambda shape: torch.empty(shape, dtype=torch.float32))
        if mutate is not None:
            mutate(eng)
        return run(eng, x, net.shift_num)


@pytest.mark.parametrize("name", list(NETS))
@pytest.mark.parametrize("run", [_run_feed, _run_lagged])
def test_unmutated_engine_gives_the_same_bits_under_both_fills(monkeypatch, name, run):
    net, st, x = _case(name)
    a, b = (_stream(monkeypatch, fill, net, st, x, run=run) for fill in (0x00, 0xFF))
    assert stale.same_bits(a, b) and not bool(torch.isnan(b).any())
    assert torch.equal(a, _run_pipeline(net, st, x))          # ... and they are the allocating pipeline's values


def test_mutant_ring_slot_read_one_step_early_is_caught(monkeypatch):
    net, st, x = _case("c16")
    a, b = (_stream(monkeypatch, fill, net, st, x, mutate=_read_early) for fill in (0x00, 0xFF))
    assert not stale.same_bits(a, b)
    assert not bool(torch.isnan(a).any())          # under zeros alone the fault computes plausible frames: one fill proves nothing


def test_mutant_producer_that_leaves_its_pad_channels_unwritten_is_caught(monkeypatch):
    net, st, x = _case("pad channels")
    a, b = (_stream(monkeypatch, fill, net, st, x, ex_cls=_PadsUnwritten) for fill in (0x00, 0xFF))
    assert not stale.same_bits(a, b)
    assert torch.equal(a, _run_pipeline(net, st, x))          # on zeroed memory the fault is invisible
    # (on the network without pad channels the same executor has nothing to leave out)
    net, st, x = _case("c16", T=3)
    a, b = (_stream(monkeypatch, fill, net, st, x, ex_cls=_PadsUnwritten) for fill in (0x00, 0xFF))
    assert stale.same_bits(a, b)


def _stub_fabric(monkeypatch, D):
    """the point-to-point stub of tests/test_dist_cpu.py: the payload moves when the RECEIVER's request is waited on"""
    mailbox = collections.defaultdict(collections.deque)
    current = {"rank": None}

    class Op:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer = op, tensor, peer

    class Req:
        def __init__(self, kind, me, op):
            self.kind, self.me, self.op = kind, me, op

        def wait(self):
            if self.kind == "recv":
                self.op.tensor.copy_(mailbox[(self.op.peer, self.me)].popleft())

    def batch(ops):
        for o in ops:
            if o.op == "isend":
                mailbox[(current["rank"], o.peer)].append(o.tensor)
        return [Req("send" if o.op == "isend" else "recv", current["rank"], o) for o in ops]

    monkeypatch.setattr(D.dist, "get_backend", lambda group=None: "nccl")
    monkeypatch.setattr(D.dist, "P2POp", Op)
    monkeypatch.setattr(D.dist, "isend", "isend")
    monkeypatch.setattr(D.dist, "irecv", "irecv")
    monkeypatch.setattr(D.dist, "batch_isend_irecv", batch)
    return current


def _sharded_layer(monkeypatch, fill, world, finish):
    """one temporal-fusion layer over ``world`` shards through dist.HaloExchanger on the stub fabric; ``finish(pending)`` -> (halo_prev, halo_next)"""
    import bsvd_amd.dist as D
    net, st, _ = _case("c16")
    sp = net.temp1["d0c1"]
    ex = OracleExecutor(st)
    v = torch.from_numpy(np.random.RandomState(3).rand(2 * world + 1, 8, 12, sp.cin_pad).astype(np.float32))
    with monkeypatch.context() as mp, stale.poisoned_empty(mp, fill, where=EVERYWHERE):
        current = _stub_fabric(mp, D)
        hx = [D.HaloExchanger(ex, r, world) for r in range(world)]
        shards = [v[a:b].contiguous() for a, b in (D.shard_range(v.shape[0], world, r) for r in range(world))]
        pend = []
        for r in range(world):
            current["rank"] = r
            pend.append(hx[r].start(sp, shards[r]))
        outs = []
        for r in range(world):
            hp, hn = finish(pend[r])
            outs.append(ex.conv(sp, shards[r], halo_prev=hp, halo_next=hn))
    return torch.cat(outs), ex.conv(sp, v)


@pytest.mark.parametrize("world", [2, 3])
def test_halo_exchange_and_its_mutant_consumed_before_the_receive_completes(monkeypatch, world):
    good = [_sharded_layer(monkeypatch, fill, world, lambda p: p.finish()) for fill in (0x00, 0xFF)]
    assert stale.same_bits(good[0][0], good[1][0]) and torch.equal(good[0][0], good[0][1])
    early = [_sharded_layer(monkeypatch, fill, world, lambda p: (p.hp, p.hn))[0] for fill in (0x00, 0xFF)]          # mutant: no wait
    assert not stale.same_bits(early[0], early[1])
