"""The soak's premise and its teeth, without a GPU (tests/soak.py; the GPU soak is tests/test_gpu_soak.py).

``StreamEngine`` runs on tests/oracle_exec.OracleExecutor through ``feed`` and ``feed_lagged`` for more than 12 ring periods of steady
state at 8 x 12.  The executor convolves in float64 and rounds every layer's output to fp32 (``double=True``): a layer's result then
does not depend on how many frames one conv2d call carries (oneDNN's fp32 blockings do, in the last bit), so the stream (one frame per
call) and the clip schedule over a window (33 frames per call) agree BIT FOR BIT -- the honest run needs no tolerance (0.0), and every
figure below is a max-abs difference against that.

* the window property holds at radius ``shift_num`` and fails at ``shift_num - 1``;
* three mutants of the ring depths, on rings that are NOT poisoned (zeros), so that only VALUES can give them away, must each fail the
  comparator at the soak's sampled indices, by more than 100 x the smallest signal the comparator is asked to resolve (the radius
  ``shift_num - 1`` leak, ~1e-7; the honest run's own tolerance is 0);
* the pool / sampling scheme visits every ring phase and every pool frame within the short form's length.
"""
import pytest
import torch

import soak
from helpers import bsvd_keys
from oracle_exec import OracleExecutor
from seeded import seeded_state
from bsvd_amd import stream_plan
from bsvd_amd.netspec import make_netspec
from bsvd_amd.schedule import bsvd_clip
from bsvd_amd.stream_plan import RING_PERIOD, StreamEngine

CHNS = [16, 32, 64]
H, W = 8, 12
PERIODS = 12


class _CpuModel:
    """what tests/soak.py asks of a model, on StreamEngine + OracleExecutor"""

    def __init__(self, poison):
        self.net = make_netspec(CHNS, CHNS[0], 4, 3, "relu6", CHNS[0])
        self.shift_num = self.net.shift_num
        self.ex = OracleExecutor(seeded_state(bsvd_keys(CHNS, CHNS[0], 4, 3, CHNS[0]), 5), double=True)
        self._stream_eng = StreamEngine(self.net, self.ex, H, W, 4, alloc=lambda shape: torch.zeros(shape, dtype=torch.float32), poison=poison)
        self.ypl = (self.net.out_ch, None)

    def feedin_one_element(self, x):
        y = self._stream_eng.feed(x, self.ypl)
        return None if y is None else y.clone()

    def feed_overlapped(self, x, last=False):
        y = self._stream_eng.feed_lagged(x, self.ypl, last=last)
        return None if y is None else y.clone()

    def reset(self):
        self._stream_eng.clear()

    def clip_forward(self, x):
        return bsvd_clip(self.ex, self.net, x, x_planar=True, y_planar=self.ypl)


def _length(shift_num):
    return 2 * shift_num + 2 * RING_PERIOD + PERIODS * RING_PERIOD + 3        # steady_start + 12 periods, ending off the period


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    """single-frame 8 x 12 convs: oneDNN's thread pool costs more than it gives (0.7 s per stream on one thread, 6 s on sixteen)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _steady(m, sample, T):
    """positions in ``sample`` of the frames that go in after the fill and come out before the first flush feed"""
    return [i for i, t in enumerate(sample) if soak.EDGE <= t < T - m.shift_num - 1]


@pytest.fixture(scope="module")
def honest(_one_thread):
    """(model, pool, T, sample, the windows' frames): computed once, shared, never written to"""
    m = _CpuModel(poison=True)
    pool = soak.Pool(4, H, W, 3)
    T = _length(m.shift_num)
    sample = soak.sample_indices(T)
    return m, pool, T, sample, soak.expected_frames(m, pool, T, sample)


def _deviation(got, want):
    d = (got.double() - want.double()).abs().flatten(1).max(dim=1).values
    return float(d.max()), int((d > 0).sum())


@pytest.mark.parametrize("api", soak.APIS)
def test_window_property_holds_at_shift_num_and_fails_one_short(honest, api):
    m, pool, T, sample, want = honest
    assert T - soak.steady_start(m) >= PERIODS * RING_PERIOD
    got, _ = soak.run_stream(m, pool, api, T, sample, mem=False)
    assert not torch.isnan(got).any()                               # poisoned rings: no slot was read before it was written
    assert torch.equal(got, want), _deviation(got, want)
    # one frame short either way: every frame is off (each with a window of its own: a block's clip would not cut its inner frames' cones)
    inner = _steady(m, sample, T)
    assert len(inner) >= 2 * RING_PERIOD
    short = torch.stack([soak.expect(m, pool, sample[i], T, radius=m.shift_num - 1) for i in inner])
    worst, n_off = _deviation(got[inner], short)
    print("%s: radius %d max-abs 0.0 on %d frames; radius %d: %.3g, %d of %d windowed frames differ"
          % (api, m.shift_num, len(sample), m.shift_num - 1, worst, n_off, len(inner)))
    assert n_off == len(inner) and worst > 0.0
    long_ = soak.expected_frames(m, pool, T, sample, radius=m.shift_num + 1)
    assert torch.equal(long_, want)


def _mutant(name):
    real = stream_plan.ring_depth

    def ring_depth(layer, is_handover=False, is_exit=False):
        if name == "tsm_feeders_2" and layer in stream_plan._TSM_FEEDERS and not is_handover and not is_exit:
            return 2
        if name == "handover_5" and is_handover:
            return 5
        if name == "inc3_5" and layer == "inc3":
            return 5
        return real(layer, is_handover, is_exit)
    return ring_depth


@pytest.mark.parametrize("api", soak.APIS)
@pytest.mark.parametrize("mutant", ["tsm_feeders_2", "handover_5", "inc3_5"])
def test_ring_depth_mutants_are_caught_by_values_alone(honest, monkeypatch, mutant, api):
    m, pool, T, sample, want = honest
    monkeypatch.setattr(stream_plan, "ring_depth", _mutant(mutant))
    bad = _CpuModel(poison=False)
    depths = {k: len(v) for k, v in bad._stream_eng.rings.items()}
    monkeypatch.undo()
    good = {k: len(v) for k, v in m._stream_eng.rings.items()}
    assert depths != good and all(RING_PERIOD % d == 0 for d in depths.values())       # the mutant keeps the period: only lifetimes break
    got, _ = soak.run_stream(bad, pool, api, T, sample, mem=False)
    assert not torch.isnan(got).any()
    worst, n_off = _deviation(got, want)
    steady = _steady(m, sample, T)
    worst_steady, n_steady = _deviation(got[steady], want[steady])
    print("mutant %-13s %-18s max-abs %.3g (%d of %d sampled frames differ; steady-state windows: %.3g, %d of %d); honest run: 0.0"
          % (mutant, api, worst, n_off, len(sample), worst_steady, n_steady, len(steady)))
    assert not torch.equal(got, want)
    assert n_steady == len(steady)                 # every steady-state sample gives it away, not only the fill
    assert worst_steady > 100 * 1e-6               # >= 100 x above anything the comparator has to resolve (1e-6 >> the 1e-7 leak; honest: 0.0)


def test_sampling_meets_every_ring_phase_and_every_pool_frame():
    """within the GPU soak's short form (>= 1000 steady-state frames after steady_start = 2 * 16 + 2 * 10)"""
    T = 2 * 16 + 2 * RING_PERIOD + 1000
    lo = 2 * 16 + 2 * RING_PERIOD
    sample = [t for t in soak.sample_indices(T) if lo <= t < T - soak.EDGE]           # the windowed samples of the steady state
    assert {t % RING_PERIOD for t in sample} == set(range(RING_PERIOD))
    assert {t % soak.POOL for t in sample} == {soak.RESIDUE}
    fed = range(lo, T)
    assert {t % soak.POOL for t in fed} == set(range(soak.POOL))
    assert len({(t % RING_PERIOD, t % soak.POOL) for t in fed}) == RING_PERIOD * soak.POOL   # every phase meets every pool frame
    # a slot stale by any multiple of the period (up to the deepest ring's reach) holds ANOTHER pool frame
    assert all((k * RING_PERIOD) % soak.POOL != 0 for k in range(1, soak.POOL))
    ends = soak.sample_indices(T)
    assert ends[:soak.EDGE] == list(range(soak.EDGE)) and ends[-soak.EDGE:] == list(range(T - soak.EDGE, T))
