"""Host logic added in round 5, on CPU: the `precision` property, the constructor-only `wide_conv`, which layer
pairs the engine may fuse (engine.pair_fusable) and the fused-pair plumbing of both schedules -- clip and the ring / plan engine -- through the
oracle-backed executor (one executor call per pair, the first conv's ring never allocated, same results as the unfused schedules)."""
import numpy as np
import pytest
import torch

from helpers import bsvd_keys, load_golden, maxabs, state_for
from oracle_exec import OracleExecutor
from seeded import seeded_state


def _model(**kw):
    import bsvd_amd
    return bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64, pretrain_ckpt=None, **kw)


def test_precision_is_a_validated_property():
    m = _model()
    assert m.precision == "f16x3" and m.precision_requested == "auto"
    m.precision = "fp32"
    assert m.precision == "fp32" and m.precision_requested == "fp32" and m._precision_init == "fp32"
    m.precision = "auto"
    assert m.precision == "f16x3"
    with pytest.raises(ValueError):
        m.precision = "bf16"
    assert m.precision == "f16x3"                  # a refused assignment changes nothing
    import bsvd_amd
    odd = bsvd_amd.BSVD(chns=[32, 40, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu", interm_ch=30, pretrain_ckpt=None)
    assert odd.precision == "fp32"                 # fold 5: 'auto' resolves to exact fp32 ...
    with pytest.raises(ValueError, match="fold"):
        odd.precision = "f16x3"                    # ... and the explicit request is refused like in the constructor
    assert odd.precision == "fp32"


def test_wide_conv_is_a_constructor_keyword_only(monkeypatch):
    from bsvd_amd import arch, engine
    monkeypatch.setenv("BSVD_WIDE_CONV", "direct")          # round 4 read this; an env leak changed the arithmetic form behind a model's back
    assert _model().wide_conv == arch.WIDE_CONV_DEFAULT == "wino2"
    assert _model(wide_conv="wino6").wide_conv == "wino6"
    assert engine.WIDE_CONV == ("direct", "wino2", "wino6", "wino26")
    with pytest.raises(ValueError):
        _model(wide_conv="wino3")
    assert _model().fuse_pairs is arch.FUSE_PAIRS_DEFAULT and _model(fuse_pairs=True).fuse_pairs is True


def test_which_pairs_are_fusable():
    from bsvd_amd.engine import pair_fusable
    from bsvd_amd.netspec import make_netspec
    net = make_netspec([64, 128, 256], 64, 4, 3, "relu6", 64)
    f = lambda S, a, b, prec="f16x3": pair_fusable(S[a], S[b], prec)       # noqa: E731
    assert not f(net.temp1, "inc0", "inc3")                  # planar 4-channel entry: that pair is the fused ENTRY (head_fusable)
    assert f(net.temp1, "out0", "out3") and f(net.temp2, "inc0", "inc3") and f(net.temp2, "out0", "out3")
    assert not f(net.temp1, "out0", "out3", "fp32")          # a split-mode kernel
    assert not f(net.temp1, "down0", "d0c1") and not f(net.temp1, "up1", "out0")      # stride 2 / temporal shift / PixelShuffle are not plain convs
    blind = make_netspec([64, 128, 256], 64, 4, 3, "relu", 30, blind=True)
    assert f(blind.temp2, "inc0", "inc3")                    # 64 -> 30 (padded 32) -> 64: one 32-channel pair
    odd = make_netspec([48, 128, 256], 48, 4, 3, "relu6", 48)
    assert not f(odd.temp1, "out0", "out3")                  # 48 mid channels: not whole 32-channel pairs


@pytest.mark.parametrize("T", [3, 7])
def test_both_schedules_with_fused_pairs_equal_the_unfused_ones(T):
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import bsvd_clip
    from bsvd_amd.stream_plan import StreamEngine
    g = load_golden("g4_bsvd_small_T%d" % T)
    st = state_for(g, bsvd_keys([32, 64, 128], 32, 4, 3, 32))
    net = make_netspec([32, 64, 128], 32, 4, 3, "relu6", 32)
    x = torch.from_numpy(g["x"][0])
    plain, fused = OracleExecutor(st), OracleExecutor(st, fuse_pairs=True)
    y0 = bsvd_clip(plain, net, x, None, x_planar=True, y_planar=(3, None))
    y1 = bsvd_clip(fused, net, x, None, x_planar=True, y_planar=(3, None))
    assert maxabs(y0.numpy(), g["out"][0]) < 1e-4 and torch.equal(y0, y1)
    assert plain.launches == 32 and fused.launches == 29     # three pairs, one call each
    assert sum("+" in k for k in fused.log) == 3
    # the ring / plan engine: the first conv of a fused pair has no ring, the pair is one recorded launch
    eng = StreamEngine(net, OracleExecutor(st, fuse_pairs=True), x.shape[2], x.shape[3], 4,
                       alloc=lambda shape: torch.zeros(shape, dtype=torch.float32), poison=True)
    for key in (net.temp1["out0"].key, net.temp2["inc0"].key, net.temp2["out0"].key):
        assert key not in eng.rings
    outs = []
    for t in range(T):
        y = eng.feed(x[t:t + 1], (3, None))
        outs.append(None if y is None else y.clone())
    for _ in range(net.shift_num):
        y = eng.feed(None, (3, None))
        outs.append(None if y is None else y.clone())
    assert eng.feed(None, (3, None)) is None
    got = torch.cat([o for o in outs if o is not None])
    assert got.shape == y0.shape and maxabs(got.numpy(), y0.numpy()) < 1e-4 and not bool(torch.isnan(got).any())      # (CPU conv2d: batch-dependent last bits)


@pytest.mark.parametrize("name,H,W,want", [("down0", 7, 9, (4, 5, 32)), ("down0", 1, 1, (1, 1, 32)),      # stride 2 at odd sizes
                                           ("up2", 3, 5, (6, 10, 32)),                                  # PixelShuffle
                                           ("out0", 4, 6, (4, 6, 16))])                                 # plain
def test_out_hwc_is_the_shape_the_oracle_conv_returns(name, H, W, want):
    """netspec.out_hwc is the one statement of a layer's output shape (executors, ring layout): it must say what a conv produces"""
    from bsvd_amd.netspec import make_netspec, out_hwc
    sp = make_netspec([16, 32, 64], 16, 4, 3, "relu6", 16).temp1[name]
    ex = OracleExecutor(seeded_state([(sp.key + ".weight", (sp.cout, sp.cin, 3, 3)), (sp.key + ".bias", (sp.cout,))], 1))
    x = torch.zeros((2, H, W, sp.cin_pad))
    y = ex.conv(sp, x)
    assert out_hwc(sp, H, W) == want
    assert tuple(y.shape) == (2,) + want == ex.out_shape(sp, x)


# the networks of tests/test_gpu_widths.py: widths off the 16 / 32 / 64 / 128 / 256 / 512 grid that the split modes accept
WIDTH_NETS = {
    "48-128-384": (dict(chns=[48, 128, 384], mid_ch=40, act="relu6", interm_ch=40), False,
                   ["d0c1", "d0c2", "d1c1", "d1c2", "u2c1", "u2c2", "up2", "u1c1", "u1c2", "up1"]),
    "80-64-128": (dict(chns=[80, 64, 128], mid_ch=48, act="relu6", interm_ch=70), False, ["d1c1", "d1c2", "u2c1", "u2c2", "up2"]),
    "96-256-512": (dict(chns=[96, 256, 512], mid_ch=64, act="relu6", interm_ch=64), False,
                   ["d0c1", "d0c2", "d1c1", "d1c2", "u2c1", "u2c2", "up2", "u1c1", "u1c2", "up1"]),
    "blind 64-128-384": (dict(chns=[64, 128, 384], mid_ch=64, act="relu", interm_ch=30, blind=True), True,
                         ["d0c1", "d0c2", "d1c1", "d1c2", "u2c1", "u2c2", "up2", "u1c1", "u1c2", "up1"]),
}


@pytest.mark.parametrize("name", list(WIDTH_NETS))
def test_networks_at_widths_off_the_power_of_two_grid(name):
    """the constructor takes them in both split modes; the entry fuses, and the Winograd form takes a layer, exactly where the netspec's widths
    say; every ring has the depth stream_plan.ring_depth states and the padded shape netspec.out_hwc states (fold 48 / 64 included);
    the ring / plan engine equals the clip schedule through the oracle-backed executor."""
    import bsvd_amd
    from bsvd_amd.engine import head_fusable, wino_eligible
    from bsvd_amd.netspec import out_hwc
    from bsvd_amd.schedule import bsvd_clip
    from bsvd_amd.stream_plan import StreamEngine, ring_depth
    kw, fused, wino = WIDTH_NETS[name]
    for precision in ("f16x3", "f16"):
        m = bsvd_amd.BSVD(in_ch=4, out_ch=3, norm="none", pretrain_ckpt=None, precision=precision, **kw)
        assert m.precision == precision
    net = m.net
    assert bsvd_amd.BSVD(in_ch=4, out_ch=3, norm="none", pretrain_ckpt=None, **kw).precision == "f16x3"          # ... and 'auto' picks the split mode
    assert head_fusable(net.temp1["inc0"], net.temp1["inc3"], "f16x3") == fused
    for blk in (net.temp1, net.temp2):
        assert [n for n, sp in blk.items() if wino_eligible(sp, "f16x3")] == wino
        assert all(sp.fold % 16 == 0 or (sp.fold == 8 and sp.cout_pad <= 64) for sp in blk.values())
        assert all(sp.cin_pad % 16 == 0 and sp.cout_pad % (64 if sp.epilogue == 1 else 16) == 0 for sp in blk.values())
    blind = kw.get("blind", False)
    st = seeded_state(bsvd_keys(kw["chns"], kw["mid_ch"], 4, 3, kw["interm_ch"], blind), 23)
    T, H, W = 5, 8, 12
    x = torch.from_numpy(np.random.RandomState(7).standard_normal((T, net.net_in_ch, H, W)).astype(np.float32))
    y0 = bsvd_clip(OracleExecutor(st, double=True), net, x, None, x_planar=True, y_planar=(3, None))
    eng = StreamEngine(net, OracleExecutor(st, double=True), H, W, net.net_in_ch, alloc=lambda shape: torch.zeros(shape, dtype=torch.float32), poison=True)
    for blk in (net.temp1, net.temp2):
        h, w = H, W
        for lname, sp in blk.items():
            h, w, c = out_hwc(sp, h, w)
            ring = eng.rings[sp.key]
            exit_ = blk is net.temp2 and lname == "out3"
            assert len(ring) == ring_depth(lname, blk is net.temp1 and lname == "out3", exit_), (lname, len(ring))
            assert tuple(ring[0].shape) == ((1, 3, h, w) if exit_ else (1, h, w, c)) and c == sp.out_channels_pad, (lname, ring[0].shape)
    outs = []
    for t in range(T + net.shift_num):
        y = eng.feed(x[t:t + 1] if t < T else None, (3, None))
        outs.append(None if y is None else y.clone())
    assert eng.feed(None, (3, None)) is None
    got = torch.cat([o for o in outs if o is not None])
    err = maxabs(got.numpy(), y0.numpy())
    print("%s: stream vs clip through the oracle-backed executor: max-abs %.2e (max |y| %.1f)" % (name, err, float(y0.abs().max())))
    assert got.shape == y0.shape and err < 1e-4 and not bool(torch.isnan(got).any())      # (the bound of the fused-pair test above)


def test_widths_the_split_modes_cannot_serve_are_refused():
    import bsvd_amd
    for precision in ("f16x3", "f16"):
        with pytest.raises(ValueError, match="fold"):      # 96- and 192-channel temporal-fusion layers: fold 12 and 24
            bsvd_amd.BSVD(chns=[48, 96, 192], mid_ch=48, norm="none", interm_ch=48, pretrain_ckpt=None, precision=precision)
    assert bsvd_amd.BSVD(chns=[48, 96, 192], mid_ch=48, norm="none", interm_ch=48, pretrain_ckpt=None).precision == "fp32"
