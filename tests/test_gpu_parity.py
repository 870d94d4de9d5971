"""Parity of the HIP path (through the C ABI) against the CPU oracle and the reference goldens.
Run on the MI355X box:  python -m pytest tests -m gpu

Tolerance: north_star asks <= 1e-3 max-abs vs the fp32 CPU forward.  The exact-fp32 mode is held to the BITS of the fmaf chain
include/bsvd_hip.h documents for it (oracle/chain_ref.c through tests/chain_exec.py) wherever a single layer is compared, and to
1e-4 max-abs against the double-accumulating oracle and the reference goldens on top (outputs are O(10))."""
import threading

import numpy as np
import pytest
import torch

from chain_exec import ChainExecutor, assert_same_bits
from helpers import load_golden, bsvd_keys, state_for, maxabs
from oracle_exec import OracleExecutor
from seeded import seeded_state, state_digest

pytestmark = pytest.mark.gpu

TOL = 1e-4
F16X3_TOL = 1.5e-4     # split-fp16 mode against the reference goldens / the CPU oracle: >= 2x the measured worst (r04: 2-6e-5 on the
                       # goldens, 8.5e-5 on the whole C1 clip; budget 1e-3)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _gpu_exec(net, st):
    from bsvd_amd.engine import HipExecutor, PackedNet
    return HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev()))


def _one_layer_net(cin, cout, stride, tsm, act, epi):
    """A NetSpec-like object holding a single layer, so PackedNet/HipExecutor can be used per layer."""
    from bsvd_amd.netspec import ConvSpec

    class One:
        pass

    sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
    o = One()
    o.layers = [sp]
    return o, sp


LAYER_CASES = [
    # cin, cout, stride, tsm, act, epi, T, H, W
    (4, 64, 1, False, "relu6", 0, 2, 20, 36),       # first layer: Cin padded 4 -> 16
    (64, 64, 1, False, "relu6", 0, 1, 33, 50),      # 256px x 64ch tile config, ragged edges
    (128, 128, 1, True, "relu6", 0, 3, 10, 19),     # temporal shift, fold 16, odd sizes
    (64, 64, 1, True, "relu6", 0, 3, 10, 19),       # fold 8: mixed first chunk on the fast path (c32-sized networks)
    (64, 64, 1, True, "relu", 0, 1, 21, 36),        # ... single frame, both halos
    (256, 256, 1, True, "relu", 0, 4, 9, 17),       # fold 32, K = 2304, 2 cout tiles
    (64, 128, 2, False, "relu6", 0, 2, 20, 36),     # stride 2
    (128, 256, 2, False, "relu6", 0, 1, 27, 43),    # stride 2, odd input size
    (32, 64, 2, False, "relu", 0, 2, 16, 24),       # stride 2, narrow Cout (masked columns)
    (256, 512, 1, False, "none", 1, 2, 9, 13),      # PixelShuffle + skip (Cq = 128)
    (128, 256, 1, False, "none", 1, 1, 12, 20),     # PixelShuffle + skip (Cq = 64)
    (64, 64, 1, False, "none", 2, 2, 12, 20),       # residual on first 3 channels, 64-ch base
    (64, 3, 1, False, "none", 2, 2, 12, 20),        # last layer: Cout 3 -> pad 16
    (24, 40, 1, True, "relu6", 0, 3, 8, 12),        # fold = 3 (not a multiple of 4): scalar gather path
    (30, 64, 1, False, "relu", 0, 1, 8, 12),        # blind net's interm_ch = 30
]


def layer_operands(cin, cout, stride, tsm, act, epi, T, H, W):
    """CPU-side operands of one LAYER_CASES / fuzz entry: (sp, net, state, x, extra, extra_pstride, [(halo_prev, halo_next), ...])"""
    from bsvd_amd.netspec import pad16
    from bsvd_amd.schedule import Halo
    rs = np.random.RandomState(cin * 1000 + cout + stride)
    st = seeded_state([("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,))], 7)
    net, sp = _one_layer_net(cin, cout, stride, tsm, act, epi)
    x = torch.zeros((T, H, W, pad16(cin)))
    x[..., :cin] = torch.from_numpy(rs.standard_normal((T, H, W, cin)).astype(np.float32))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    extra, eps = None, 0
    if epi == 1:
        cqp = sp.cout_pad // 4
        extra = torch.zeros((T, 2 * Ho, 2 * Wo, cqp))
        extra[..., :cout // 4] = torch.from_numpy(rs.standard_normal((T, 2 * Ho, 2 * Wo, cout // 4)).astype(np.float32))
        eps = cqp
    elif epi == 2:
        extra = torch.from_numpy(rs.standard_normal((T, Ho, Wo, 16)).astype(np.float32))
        eps = 16
    halos = [(None, None)]
    if tsm:
        fold = sp.fold
        hp = torch.from_numpy(rs.standard_normal((H, W, fold)).astype(np.float32))
        hn = torch.from_numpy(rs.standard_normal((H, W, fold)).astype(np.float32))
        full = torch.from_numpy(rs.standard_normal((1, H, W, pad16(cin))).astype(np.float32))
        halos += [(Halo(hp, fold, 0), Halo(hn, fold, 0)), (Halo(full, pad16(cin), fold), Halo(full, pad16(cin), 0))]
    return sp, net, st, x, extra, eps, halos


@pytest.mark.parametrize("cin,cout,stride,tsm,act,epi,T,H,W", LAYER_CASES)
def test_layer_vs_oracle(cin, cout, stride, tsm, act, epi, T, H, W):
    """Within TOL of the double-accumulating oracle AND the bits of the documented fmaf chain (the 50 seeds of
    test_gpu_fuzz.py::test_random_layer_exact_fp32 come through here too)."""
    from bsvd_amd.schedule import Halo
    sp, net, st, x, extra, eps, halos = layer_operands(cin, cout, stride, tsm, act, epi, T, H, W)
    gex, oex, cex = _gpu_exec(net, st), OracleExecutor(st, double=True), ChainExecutor(st)
    for hp, hn in halos:
        want = oex.conv(sp, x, hp, hn, extra, eps, 1)
        d = lambda h: None if h is None else Halo(h.t.to(_dev()), h.pstride, h.coff)
        got = gex.conv(sp, x.to(_dev()), d(hp), d(hn), None if extra is None else extra.to(_dev()), eps, 1)
        torch.cuda.synchronize()
        assert got.shape == want.shape
        assert maxabs(got.cpu().numpy(), want.numpy()) < TOL
        assert_same_bits(got, cex.conv(sp, x, hp, hn, extra, eps, 1), "%s, halos %s" % (sp, "none" if hp is None else hp.pstride))


EDGE_CASES = [
    # kind, cin, cout, act, T, H, W
    ("head", 4, 64, "relu6", 2, 21, 70),
    ("head", 3, 30, "relu", 1, 9, 130),
    ("head", 4, 32, "none", 3, 4, 8),
    ("tail", 64, 3, "none", 2, 21, 37),
    ("tail", 32, 3, "none", 1, 16, 16),
    ("tail", 64, 4, "relu", 2, 5, 50),
]


def edge_operands(kind, cin, cout, act, T, H, W):
    """CPU-side operands of one EDGE_CASES entry: (sp, net, state, x, [conv keywords, ...])"""
    from bsvd_amd.netspec import pad16
    rs = np.random.RandomState(cin * 100 + cout + H)
    st = seeded_state([("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,))], 9)
    epi = 0 if kind == "head" else 2
    net, sp = _one_layer_net(cin, cout, 1, False, act, epi)
    if kind == "head":
        x = torch.from_numpy(rs.standard_normal((T, cin, H, W)).astype(np.float32))
        return sp, net, st, x, [dict(x_planar=True)]
    x = torch.zeros((T, H, W, pad16(cin)))
    x[..., :cin] = torch.from_numpy(rs.standard_normal((T, H, W, cin)).astype(np.float32))
    base_planar = torch.from_numpy(rs.standard_normal((T, 4, H, W)).astype(np.float32))
    base_nhwc = torch.from_numpy(rs.standard_normal((T, H, W, 64)).astype(np.float32))
    kws = [dict(extra=base, extra_pstride=eps, extra_cstride=ecs, y_planar=(cout, clamp))
           for base, eps, ecs in ((base_planar, 1, H * W), (base_nhwc, 64, 1)) for clamp in (None, (0.0, 1.0))]
    return sp, net, st, x, kws


@pytest.mark.parametrize("kind,cin,cout,act,T,H,W", EDGE_CASES)
def test_edge_layers_vs_oracle(kind, cin, cout, act, T, H, W):
    """First layer reading the planar NCHW input, last layer writing planar NCHW with residual (+clamp): within TOL of the
    double-accumulating oracle and the bits of the documented fmaf chain."""
    from bsvd_amd.netspec import pad16
    sp, net, st, x, kws = edge_operands(kind, cin, cout, act, T, H, W)
    gex, oex, cex = _gpu_exec(net, st), OracleExecutor(st, double=True), ChainExecutor(st)
    for kw in kws:
        want = oex.conv(sp, x, **kw)
        got = gex.conv(sp, x.to(_dev()), **{k: v.to(_dev()) if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
        assert got.shape == want.shape == ((T, H, W, pad16(cout)) if kind == "head" else (T, cout, H, W))
        assert maxabs(got.cpu().numpy(), want.numpy()) < TOL
        assert_same_bits(got, cex.conv(sp, x, **kw), "%s %s" % (kind, kw.get("y_planar")))


def test_layout_roundtrip_and_clamp():
    net, sp = _one_layer_net(16, 16, 1, False, "none", 0)
    gex = _gpu_exec(net, seeded_state([("l.weight", (16, 16, 3, 3)), ("l.bias", (16,))], 1))
    x = torch.randn(3, 5, 14, 22)
    n = gex.to_nhwc(x.to(_dev()), 16)
    assert torch.equal(n[..., :5].cpu(), x.permute(0, 2, 3, 1)) and float(n[..., 5:].abs().max()) == 0
    assert torch.equal(gex.to_nchw(n, 5).cpu(), x)
    assert torch.equal(gex.to_nchw(n, 3, (0.0, 1.0)).cpu(), x[:, :3].clamp(0, 1))
    assert torch.equal(gex.halo_pack(n[1], 2, 3).cpu(), x[1, 2:5].permute(1, 2, 0))


def _module(chns, mid_ch, interm_ch, act, st, blind=False, mode="clip"):
    import bsvd_amd
    m = bsvd_amd.BSVD(precision="fp32", chns=chns, mid_ch=mid_ch, in_ch=4, out_ch=3, norm="none", act=act, interm_ch=interm_ch,
                      blind=blind, pretrain_ckpt=None, engine_mode=mode)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(_dev())


@pytest.mark.parametrize("T", [1, 2, 3, 7])
def test_golden_small_net(T):
    g = load_golden("g4_bsvd_small_T%d" % T)
    st = state_for(g, bsvd_keys([32, 64, 128], 32, 4, 3, 32))
    x = torch.from_numpy(g["x"]).to(_dev())
    yc = _module([32, 64, 128], 32, 32, "relu6", st, mode="clip")(x)
    ys = _module([32, 64, 128], 32, 32, "relu6", st, mode="stream")(x)
    assert maxabs(yc.cpu().numpy(), g["out"]) < TOL
    assert maxabs(ys.cpu().numpy(), g["out"]) < TOL
    assert torch.equal(yc, ys), "clip and stream schedules run the same kernels on the same operands"


def test_golden_batch_of_clips_is_one_long_clip():
    """N = 2 (recorded from the real reference forward): frames of different batch items are temporal neighbours."""
    g = load_golden("g4c_batch_is_one_clip")
    st = state_for(g, bsvd_keys([32, 64, 128], 32, 4, 3, 32))
    x = torch.from_numpy(g["x"]).to(_dev())
    for mode in ("clip", "stream"):
        y = _module([32, 64, 128], 32, 32, "relu6", st, mode=mode)(x)
        assert tuple(y.shape) == g["out"].shape and maxabs(y.cpu().numpy(), g["out"]) < TOL


@pytest.mark.parametrize("mode", ["clip", "stream"])
def test_reset_after_an_unfinished_stream_gives_a_fresh_stream(mode):
    """Deliberate deviation: in the reference, reset() after three un-flushed feeds leaves stale skip
    frames behind and the next clips come out wrong (golden g4d: `dirty`, `again` != `clean`).  Here the same call
    sequence returns the clean result in both schedules."""
    g = load_golden("g4d_reset_mid_stream")
    assert bool(g["differs"]) and not bool(g["again_clean"])           # what the real reference does
    st = state_for(g, bsvd_keys([32, 64, 128], 32, 4, 3, 32))
    m = _module([32, 64, 128], 32, 32, "relu6", st, mode=mode)
    pre, x = torch.from_numpy(g["pre"]).to(_dev()), torch.from_numpy(g["x"]).to(_dev())
    assert maxabs(m(x).cpu().numpy(), g["clean"]) < TOL
    for t in range(3):
        assert m.feedin_one_element(pre[0, t:t + 1]) is None
    m.reset()
    assert maxabs(m(x).cpu().numpy(), g["clean"]) < TOL
    assert maxabs(m(x).cpu().numpy(), g["clean"]) < TOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_golden_default_ctor_odd_channels(precision):
    """The reference constructor's own defaults (chns [32,64,128], mid_ch 3, interm_ch 30, ReLU) with norm='none'."""
    import bsvd_amd
    g = load_golden("g4b_bsvd_defaults")
    st = state_for(g, bsvd_keys([32, 64, 128], 3, 4, 3, 30))
    x = torch.from_numpy(g["x"]).to(_dev())
    m = bsvd_amd.BSVD(norm="none", pretrain_ckpt=None, precision=precision)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    m = m.to(_dev())
    y = m(x[:, :, :3], noise_map=x[:, :, 3:4])
    err = maxabs(y.cpu().numpy(), g["out"])
    print("reference-default ctor, %s: max-abs vs golden %.2e" % (precision, err))
    assert err < (TOL if precision == "fp32" else F16X3_TOL)      # measured 2.0e-5
    m.engine_mode = "stream"
    assert torch.equal(m(x[:, :, :3], noise_map=x[:, :, 3:4]), y)


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_golden_reference_default_constructor_with_batchnorm(precision):
    """BSVD() exactly as the reference constructs it by default (norm='bn', bsvd_arch.py:446) in eval mode with non-trivial
    BatchNorm affine parameters and running statistics (golden g13): folded into the packed conv weights at pack time."""
    import bsvd_amd
    g = load_golden("g13_batchnorm_defaults")
    st = state_for(g, bsvd_keys([32, 64, 128], 3, 4, 3, 30, norm="bn"))
    m = bsvd_amd.BSVD(pretrain_ckpt=None, precision=precision)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st.items()})
    m = m.to(_dev())
    x = torch.from_numpy(g["x"]).to(_dev())
    with pytest.raises(RuntimeError, match="eval"):
        m(x)
    m.eval()
    assert m.precision == ("fp32" if precision == "fp32" else "f16x3")
    y = m(x)
    scale = float(np.abs(g["out"]).max())
    err = maxabs(y.cpu().numpy(), g["out"])
    print("BSVD() with norm='bn', %s: max-abs vs golden %.2e at output magnitude %.1f" % (m.precision, err, scale))
    assert err < (2e-5 if m.precision == "fp32" else 5e-5) * scale
    m.engine_mode = "stream"
    assert torch.equal(m(x), y)
    with torch.no_grad():                           # a changed running statistic re-packs the folded weights
        m.temp1.inc.convblock["1"].running_mean.add_(0.25)
    assert not torch.equal(m(x), y)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_golden_c64(tag):
    g = load_golden("g5_bsvd_c64_" + tag)
    st = state_for(g, bsvd_keys([64, 128, 256], 64, 4, 3, 64))
    m = _module([64, 128, 256], 64, 64, "relu6", st)
    y = m(torch.from_numpy(g["x"]).to(_dev()))
    assert maxabs(y.cpu().numpy(), g["out"]) < TOL
    if tag in ("c", "d"):
        m.engine_mode = "stream"
        assert maxabs(m(torch.from_numpy(g["x"]).to(_dev())).cpu().numpy(), g["out"]) < TOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_golden_blind_from_tsn_checkpoint(tmp_path, precision):
    """BASELINE config 3 (blind bsvd_c64: interm_ch = 30, unbounded ReLU) from a TSN-schema checkpoint, both arithmetic
    modes: in the split mode the 30-channel tensors ride on two zero padding channels."""
    from bsvd_amd import checkpoint
    g = load_golden("g6_blind_c64")
    tsn = seeded_state([(k, tuple(int(v) for v in s.split(","))) for k, s in zip(g["tsn_keys"], g["tsn_shapes"])],
                       int(g["seed"]))
    assert state_digest(tsn) == str(g["digest"])
    p = tmp_path / "tsn.pth"
    torch.save({"params": {"module." + k: torch.from_numpy(v) for k, v in tsn.items()}}, p)
    import bsvd_amd
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu", interm_ch=30, blind=True,
                      pretrain_ckpt=str(p), precision=precision).to(_dev())
    y = m(torch.from_numpy(g["x"]).to(_dev()))
    err = maxabs(y.cpu().numpy(), g["out"])
    print("blind c64 %s max-abs vs the reference golden: %.2e" % (precision, err))
    assert err < (TOL if precision == "fp32" else F16X3_TOL)      # measured 3.9e-5
    m.engine_mode = "stream"
    assert torch.equal(m(torch.from_numpy(g["x"]).to(_dev())), y)


def test_feedin_one_element_protocol():
    """None-in/None-out protocol and 16-step latency of the streaming API (bsvd_arch.py:485-552)."""
    g = load_golden("g4_bsvd_small_T3")
    st = state_for(g, bsvd_keys([32, 64, 128], 32, 4, 3, 32))
    m = _module([32, 64, 128], 32, 32, "relu6", st, mode="stream")
    x = torch.from_numpy(g["x"][0]).to(_dev())
    sched, outs = [], []
    for v in [x[i:i + 1] for i in range(3)] + [None] * 17:
        y = m.feedin_one_element(v)
        sched.append([v is None, y is None])
        if y is not None:
            outs.append(y)
    assert sched == [list(map(bool, s)) for s in g["schedule"]]
    assert maxabs(torch.cat(outs).cpu().numpy(), g["out"][0]) < TOL
    m.reset()


def test_sharded_equals_unsharded_bitwise():
    """Two frame-window shards with per-layer halos == the unsharded clip, bit for bit."""
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import Halo, bsvd_clip
    g = load_golden("g5_bsvd_c64_a")
    st = state_for(g, bsvd_keys([64, 128, 256], 64, 4, 3, 64))
    net = make_netspec([64, 128, 256], 64, 4, 3, "relu6", 64)
    x = torch.from_numpy(g["x"][0]).to(_dev())
    ex = _gpu_exec(net, st)
    whole = ex.to_nchw(bsvd_clip(ex, net, ex.to_nhwc(x, 16)), 3)
    boxes, results = {}, [None, None]
    barrier = threading.Barrier(2)

    def rank(r, frames):
        torch.cuda.set_device(0)
        e = _gpu_exec(net, st)

        class ThreadHalo:
            """Two lock-stepped 'ranks' on one GPU.  start()/finish() exercises the overlapped schedule
            (interior frames first, writes into frame ranges of one output tensor) for shards of >= 3 frames."""

            def start(self, sp, v):
                fold = sp.fold
                boxes[(r, sp.key)] = (e.halo_pack(v[0], 0, fold), e.halo_pack(v[-1], fold, fold))

                class P:
                    def finish(self_p):
                        torch.cuda.synchronize()
                        barrier.wait()
                        other = boxes[(1 - r, sp.key)]
                        barrier.wait()
                        return (None, Halo(other[0], fold, 0)) if r == 0 else (Halo(other[1], fold, 0), None)
                return P()

            def __call__(self, sp, v):
                return self.start(sp, v).finish()

        results[r] = e.to_nchw(bsvd_clip(e, net, e.to_nhwc(frames, 16), ThreadHalo()), 3)
        torch.cuda.synchronize()

    th = [threading.Thread(target=rank, args=(0, x[:2])), threading.Thread(target=rank, args=(1, x[2:]))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert torch.equal(torch.cat(results), whole)
    assert maxabs(whole.cpu().numpy(), g["out"][0]) < TOL


def test_full_resolution_two_frames_vs_oracle():
    """BASELINE config 1 geometry (540x960, bsvd_c64), 2 frames: HIP vs the torch CPU oracle."""
    from oracle import bsvd_oracle as O
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 11)
    from seeded import seeded_clip
    x = torch.from_numpy(seeded_clip((1, 2, 4, 540, 960), 12, kind="sigma30"))
    m = _module([64, 128, 256], 64, 64, "relu6", st)
    y = m(x.to(_dev())).cpu()
    want = O.bsvd_clip(x, O.to_torch_state(st))
    assert maxabs(y.numpy(), want.numpy()) < 1e-3
    m.engine_mode = "stream"
    assert torch.equal(m(x.to(_dev())).cpu(), y)


def test_denoising_model_pad_clamp_crop_end_to_end():
    """DenoisingModel.test() protocol (denoising_model.py:170-190) on a 30x50 clip (not a multiple of 4):
    reflect pad -> whole clip in one call with a constant noise map -> clamp -> crop, vs the CPU oracle."""
    import torch.nn.functional as F
    import bsvd_amd
    from oracle import bsvd_oracle as O
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32), 21)
    opt = {"is_train": False, "num_gpu": 1, "val": {"temp_psz": -1},
           "network_g": {"type": "BSVD", "chns": [32, 64, 128],
                         "mid_ch": 32, "shift_input": False, "in_ch": 4, "out_ch": 3, "norm": "none", "act": "relu6",
                         "interm_ch": 32, "blind": False, "pretrain_ckpt": None}}
    model = bsvd_amd.MODEL_REGISTRY.get("DenoisingModel_MI355X")(opt)
    model.net_g.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    rs = np.random.RandomState(22)
    gt = torch.from_numpy(rs.uniform(0, 1, (6, 3, 30, 50)).astype(np.float32))
    lq = gt + torch.from_numpy(rs.standard_normal(gt.shape).astype(np.float32)) * (30 / 255.0)
    nm = torch.full((6, 1, 30, 50), 30 / 255.0)
    model.feed_data({"lq": lq, "gt": gt, "noise_map": nm})
    model.test()
    got = model.get_current_visuals()["result"]
    assert got.shape == (1, 6, 3, 30, 50)
    pl = F.pad(lq, (0, 2, 0, 2), mode="reflect")
    pn = torch.full((1, 6, 1, 32, 52), 30 / 255.0)
    cfg = O.default_cfg(chns=[32, 64, 128], mid_ch=32, interm_ch=32)
    want = O.bsvd_clip(pl[None], O.to_torch_state(st), cfg, noise_map=pn).clamp(0, 1)[..., :30, :50]
    assert maxabs(got.numpy(), want.numpy()) < TOL


@pytest.mark.parametrize("tag", ["a", "c", "d"])
def test_tsn_segmented_inference_on_gpu(tag):
    """MIMO mode on the HIP engine: TSN + denoise_seq (segments, look-ahead, mirrored tail, queued past slices)."""
    import bsvd_amd
    from bsvd_amd.arch import TSN
    g = load_golden("g10_mimo_segments")
    st = seeded_state([(str(k), tuple(int(v) for v in str(s_).split(","))) for k, s_ in zip(g["tsn_keys"], g["tsn_shapes"])],
                      int(g["seed"]))
    m = TSN(precision="fp32", num_segments=3, net2d_opt=dict(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6",
                                           interm_ch=32, blind=False))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m = m.to(_dev()).eval()
    T, psz, fbl = (int(v) for v in g["cfg_" + tag])
    seq = torch.from_numpy(g["seq_" + tag])
    nm = torch.full((T, 1) + tuple(seq.shape[-2:]), 30.0 / 255.0)
    den = bsvd_amd.denoise_seq(seq, nm, psz, m, future_buffer_len=fbl)
    assert maxabs(den.numpy(), g["den_" + tag]) < TOL


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_tsn_blind_whole_clip_on_gpu(precision):
    """The blind c64 checkpoint schema through the TSN class (what the reference runs for blind denoising)."""
    from bsvd_amd.arch import TSN
    from bsvd_amd import global_queue_buffer as gq
    g = load_golden("g6_blind_c64")
    st = seeded_state([(str(k), tuple(int(v) for v in str(s_).split(","))) for k, s_ in zip(g["tsn_keys"], g["tsn_shapes"])],
                      int(g["seed"]))
    m = TSN(num_segments=5, net2d_opt=dict(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu",
                                           interm_ch=30, blind=True), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m = m.to(_dev()).eval()
    gq._init(0)
    gq.set_batch_index(0)
    y = m(torch.from_numpy(g["x"]).to(_dev()))
    gq._clean()
    assert maxabs(y.cpu().numpy(), g["out"]) < (TOL if precision == "fp32" else F16X3_TOL)


@pytest.mark.parametrize("shape", [(1, 1, 4, 4, 4), (1, 2, 4, 8, 4), (2, 3, 4, 12, 20), (1, 1, 4, 4, 132)])
def test_tiny_and_ragged_clips_vs_oracle(shape):
    """Smallest legal frames (4x4: every level is a single masked tile), one-frame clips, N > 1 (the reference treats
    the batch as one long clip, bsvd_arch.py:494-496), tiles with ragged right/bottom edges -- both arithmetic modes."""
    from oracle import bsvd_oracle as O
    from seeded import seeded_clip
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 51)
    x = torch.from_numpy(seeded_clip(shape, 52))
    want = O.bsvd_clip(x, O.to_torch_state(st))
    import bsvd_amd
    for precision, tol in (("fp32", TOL), ("f16x3", F16X3_TOL)):
        for mode in ("clip", "stream"):
            m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu6", interm_ch=64, pretrain_ckpt=None,
                              engine_mode=mode, precision=precision)
            m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
            y = m.to(_dev())(x.to(_dev()))
            assert y.shape == want.shape
            assert maxabs(y.cpu().numpy(), want.numpy()) < tol, (precision, mode)


def test_half_io_like_profile_py():
    """profile.py calls net_g.half() and feeds fp16 under autocast (profile.py:79-83): fp16 in, fp16 out, fp32 inside."""
    import bsvd_amd
    from oracle import bsvd_oracle as O
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 53)
    m = bsvd_amd.BSVD(precision="fp32", chns=[64, 128, 256], mid_ch=64, norm="none", act="relu6", interm_ch=64, pretrain_ckpt=None)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    m = m.to(_dev()).half().eval()
    x = torch.randn(1, 3, 4, 16, 24).half()
    with torch.autocast("cuda", enabled=True):
        y = m(x.to(_dev()))
    assert y.dtype == torch.float16 and y.shape == (1, 3, 3, 16, 24)
    P = {k: v.half().float() for k, v in O.to_torch_state(st).items()}        # .half() rounded the weights
    want = O.bsvd_clip(x.float(), P)
    assert maxabs(y.float().cpu().numpy(), want.numpy()) < 2e-2                # fp16 output rounding at |y| ~ 10


def test_uint8_frame_io_on_device():
    """uint8 ingest (+ constant sigma channel) and uint8 output with the reference's clamp + round-half-even."""
    from bsvd_amd import frame_io
    from bsvd_amd.evaluation import tensor2img
    rs = np.random.RandomState(61)
    u8 = torch.from_numpy(rs.randint(0, 256, (3, 10, 14, 3)).astype(np.uint8))
    x = frame_io.frames_to_input(u8.to(_dev()), sigma=30 / 255.0)
    want = torch.cat([torch.from_numpy(np.float32(u8.numpy().transpose(0, 3, 1, 2) / 255.)),
                      torch.full((3, 1, 10, 14), 30 / 255.0)], dim=1)
    assert torch.equal(x.cpu(), want)
    assert torch.equal(frame_io.frames_to_input(u8.permute(0, 3, 1, 2).contiguous().to(_dev()), hwc=False).cpu(), want[:, :3])
    y = torch.from_numpy(rs.uniform(-0.2, 1.2, (3, 3, 10, 14)).astype(np.float32))
    y[0, 0, 0, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255])         # ties -> even
    got = frame_io.output_to_frames(y.to(_dev()), rgb2bgr=True).cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f], tensor2img(y[f]))                                 # HWC, BGR, rounded like the reference
    assert np.array_equal(frame_io.output_to_frames(y.to(_dev()), hwc=False).cpu().numpy(),
                          (y.clamp(0, 1).numpy() * 255.0).round().astype(np.uint8))


def test_halo_unpack_materialised_neighbours_equal_halo_slices():
    """bsvd_halo_unpack is the inverse of bsvd_halo_pack, and a temporal-fusion conv fed compact halo slices equals the
    same conv fed full neighbour frames the slices were unpacked into (the reference's materialised buffers)."""
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    net, sp = _one_layer_net(128, 128, 1, True, "relu6", 0)
    rs = np.random.RandomState(3)
    st = {"l.weight": (rs.standard_normal((128, 128, 3, 3)) * 0.03).astype(np.float32),
          "l.bias": rs.standard_normal(128).astype(np.float32) * 0.1}
    ex = _gpu_exec(net, st)
    x = torch.from_numpy(rs.standard_normal((3, 10, 19, 128)).astype(np.float32)).to(_dev())
    fold = sp.fold
    prev_slice = ex.halo_pack(x[0], fold, fold)
    next_slice = ex.halo_pack(x[2], 0, fold)
    assert torch.equal(prev_slice, x[0, :, :, fold:2 * fold]) and torch.equal(next_slice, x[2, :, :, :fold])
    prev_full = torch.full_like(x[0], 7.0)
    next_full = torch.full_like(x[0], -7.0)
    ex.halo_unpack(prev_slice, prev_full, fold)
    ex.halo_unpack(next_slice, next_full, 0)
    assert torch.equal(prev_full[:, :, fold:2 * fold], prev_slice) and bool((prev_full[:, :, :fold] == 7.0).all())
    assert torch.equal(next_full[:, :, :fold], next_slice) and bool((next_full[:, :, fold:] == -7.0).all())
    mid = x[1:2].contiguous()
    y_slices = ex.conv(sp, mid, halo_prev=Halo(prev_slice, fold, 0), halo_next=Halo(next_slice, fold, 0))
    y_full = ex.conv(sp, mid, halo_prev=Halo(prev_full, 128, fold), halo_next=Halo(next_full, 128, 0))
    y_clip = ex.conv(sp, x)[1:2]
    assert torch.equal(y_slices, y_full) and torch.equal(y_slices, y_clip)


def test_rejects_bad_arguments():
    from bsvd_amd import _lib
    import ctypes
    lib = _lib.load()
    a = _lib.BsvdConvArgs()
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) < 0
    assert b"non-NULL" in lib.bsvd_last_error()
    import bsvd_amd
    m = bsvd_amd.BSVD(precision="fp32", norm="none", pretrain_ckpt=None).to(_dev())
    with pytest.raises(ValueError):
        m(torch.zeros(1, 2, 4, 18, 26, device=_dev()))     # not a multiple of 4 (reference fails at the skip add)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 0, 4, 16, 16, device=_dev()))     # empty clip (reference: torch.cat of nothing)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 2, 5, 16, 16, device=_dev()))     # wrong channel count
    # the executor refuses host tensors / wrong dtypes instead of handing their pointers to a kernel
    net, sp = _one_layer_net(64, 64, 1, False, "relu6", 0)
    rs = np.random.RandomState(0)
    ex = _gpu_exec(net, {"l.weight": rs.standard_normal((64, 64, 3, 3)).astype(np.float32), "l.bias": np.zeros(64, np.float32)})
    with pytest.raises(ValueError):
        ex.conv(sp, torch.zeros(1, 8, 8, 64))
    with pytest.raises(ValueError):
        ex.conv(sp, torch.zeros(1, 8, 8, 64, device=_dev(), dtype=torch.float16))
    with pytest.raises(ValueError):
        ex.conv(sp, torch.zeros(1, 8, 8, 64, device=_dev()), out=torch.zeros(1, 8, 8, 64))
