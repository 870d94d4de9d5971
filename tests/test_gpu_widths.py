"""Split-mode layers and whole networks at channel widths OFF the 16 / 32 / 64 / 128 / 256 / 512 grid every other split-mode GPU test draws
from: Cout 48, 80, 96, 192, 320, 384 (a 64- or 128-channel tile partly live; Cout % 32 == 16: a 32-channel granule half live), K loops of
3, 5, 6, 9, 24 and 32 chunks (the chunk-parity double buffers; the zero-chunk skip with fold 48 and 64), PixelShuffle with Cout / 4 of 48, 80,
96 and a skip tensor of that width, the stride-2 tile at Cout 64 / 256 / 384, real channel counts that ride on zero padding channels (40 -> 70),
and the networks bsvd_amd.BSVD builds from such widths: chns [48,128,384], [80,64,128], [96,256,512] and the blind [64,128,384].

No tolerance is introduced here: the layer cases call the checkers of test_gpu_f16x3 (flat TIGHT against the double-accumulating oracle AND
split_model.needed <= M_DIRECT against the three-pass model), test_gpu_wino (both product forms, M_WINO) and test_gpu_f32_handover; the
networks are held to TOL of test_gpu_f16x3 (1e-3) and, in precision='f16', to twice the CPU emulation's error like test_gpu_f16.  Every case
asserts through HipExecutor.last_variant that it ran the tile family it was written for.  Measured figures: profiles/channel_widths.txt
(the `WIDTHS |` lines this file prints).
"""
import threading

import numpy as np
import pytest
import torch

import split_model as S
import test_gpu_f16x3 as X3
import test_gpu_wino as WN
from helpers import bsvd_keys, maxabs
from oracle_exec import OracleExecutor
from seeded import seeded_state

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _table(tag, rows):
    for case, halo, variant, err, need, m in rows:
        print("WIDTHS | %s | %s | halo %s | %s | max-abs %.3e | needs %.3f of %d" % (tag, case, halo, variant, err, need, m))


# ---------------------------------------------------------------------------------------------------------------------------------------
# direct form

NARROW, WIDE, FAT, STRIDE2 = ("conv3x3_kernel<4,1,2,2,1>[f16x3]", "conv3x3_kernel<2,2,2,2,1>[f16x3]", "conv3x3_kernel<4,2,2,2,1>[f16x3]",
                              "conv3x3_kernel<4,1,1,4,2>[f16x3]")
DIRECT = [
    # cin, cout (REAL channel counts), stride, tsm, act, epi, T, H, W, the tile family
    (48, 48, 1, False, "relu6", 0, 2, 21, 37, NARROW),        # 3 chunks; the second 32-channel granule of the 64-channel tile half live
    (40, 70, 1, False, "relu", 0, 1, 33, 37, WIDE),           # pads to 48 -> 80: padding channels on both sides, 80 of 128 tile channels
    (80, 80, 1, False, "relu6", 0, 2, 20, 24, WIDE),          # 5 chunks
    (96, 96, 1, False, "none", 0, 2, 17, 21, WIDE),           # 6 chunks, 96 of 128
    (64, 96, 1, False, "relu6", 0, 1, 21, 37, WIDE),
    (128, 192, 1, False, "relu6", 0, 2, 20, 24, WIDE),        # two channel tiles, the second half live
    (48, 128, 2, False, "relu6", 0, 2, 21, 37, STRIDE2),
    (80, 64, 2, False, "relu6", 0, 2, 18, 36, STRIDE2),       # half of the 128-channel stride-2 tile masked
    (96, 256, 2, False, "relu6", 0, 1, 27, 43, STRIDE2),
    (128, 384, 2, False, "relu6", 0, 1, 21, 19, STRIDE2),
    (128, 192, 1, False, "none", 1, 1, 17, 21, WIDE),         # PixelShuffle: Cout / 4 = 48, the generic item addressing
    (64, 320, 1, False, "none", 1, 2, 9, 13, WIDE),           # Cout / 4 = 80
    (256, 384, 1, False, "none", 1, 1, 12, 20, WIDE),         # Cout / 4 = 96: the wave-uniform item addressing at a width that is not a power of two
    (64, 280, 1, False, "none", 1, 1, 9, 13, WIDE),           # Cout / 4 = 70 real channels in 80: padding channels of y behind a padded skip tensor
    (384, 384, 1, True, "relu6", 0, 3, 10, 19, WIDE),         # fold 48: 24 chunks, three per temporal source
    (512, 512, 1, True, "relu", 0, 2, 9, 17, WIDE),           # fold 64: 32 chunks, four per temporal source
]
DIRECT_RUNS = [c[:9] + (0, c[9]) for c in DIRECT] + [c[:9] + (1, FAT) for c in DIRECT if c[9] == WIDE]


@pytest.mark.parametrize("cin,cout,stride,tsm,act,epi,T,H,W,fat,variant", DIRECT_RUNS)
def test_direct_layer_vs_oracle_and_three_pass_model(cin, cout, stride, tsm, act, epi, T, H, W, fat, variant):
    """test_gpu_f16x3.test_layer_split_vs_oracle (which walks all three halo forms of a temporal-fusion layer and holds the padding channels of
    the result to exact zeros); the wide layers a second time on the 128-accumulator tile (HipExecutor.fat_min_wgs = 1), where the layers with
    a temporal shift leave the all-zero chunks of fold 48 / 64 out of their K loops."""
    rows = X3.check_layer_split(cin, cout, stride, tsm, act, epi, T, H, W, fat=fat, variant=variant)
    assert len(rows) == (3 if tsm else 1) and all(r[2] == variant for r in rows)
    _table("direct", rows)


@pytest.mark.parametrize("cin", [48, 80])
def test_planar_exit_with_a_split_base(cin):
    """the network's exit layer Cin -> 3, RESID with a split16 residual base, planar clamped output: 3 and 5 chunks through the 256-px x 32-ch tile"""
    import ctypes
    from test_gpu_strides import _args, _layer
    c = _layer("f16x3", cin, 3, 1, False, "none", 2, 2, 21, 37, "none", "split64", (3, (0.0, 1.0)))
    a, y = _args(c)
    buf = ctypes.create_string_buffer(128)
    assert c.ex.lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 128) == 0
    assert buf.value.decode() == "conv3x3_kernel<2,1,4,1,1>[f16x3][planar out]", buf.value
    assert c.ex.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    err = maxabs(y.cpu().numpy(), c.ref.numpy())
    print("WIDTHS | exit | %d -> 3 RESID, split base | %s | max-abs %.3e (bound %.1e)" % (cin, buf.value.decode(), err, c.tol))
    assert y.shape == c.ref.shape and err < c.tol


@pytest.mark.parametrize("cin,cmid,cout,act,T,H,W", [(4, 96, 64, "relu6", 2, 20, 36), (3, 32, 48, "relu", 2, 17, 21)])
def test_fused_entry(cin, cmid, cout, act, T, H, W, monkeypatch):
    """three chunk pairs of the first conv (Cmid 96); a second conv whose 64-channel tile is three quarters live (Cout 48)"""
    X3.test_fused_entry_vs_two_step_oracle_and_vs_the_unfused_kernels(cin, cmid, cout, act, T, H, W, monkeypatch)


def test_unfused_entry_for_a_middle_width_that_is_no_whole_chunk_pair():
    """interm_ch = 40 pads to 48: not whole 32-channel pairs, so engine.head_fusable declines and InputCvBlock runs as its two launches --
    the fp32 VALU entry kernel writing pairs (padding channels 40 .. 47 exact zeros) and the narrow tile at Cin = Cout = 48.  Each against
    the oracle on the operands it reads, and the block against the oracle's two convs."""
    from types import SimpleNamespace
    from bsvd_amd.engine import HipExecutor, PackedNet, head_fusable
    from bsvd_amd.netspec import ConvSpec
    T, H, W = 2, 21, 37
    sp0 = ConvSpec("inc0", "b.inc.convblock.0", 4, 40, 1, False, "relu6", 0)
    sp3 = ConvSpec("inc3", "b.inc.convblock.3", 40, 48, 1, False, "relu6", 0)
    net = SimpleNamespace(layers=[sp0, sp3], temp1={"inc0": sp0, "inc3": sp3})
    st = seeded_state([(sp0.key + ".weight", (40, 4, 3, 3)), (sp0.key + ".bias", (40,)), (sp3.key + ".weight", (48, 40, 3, 3)), (sp3.key + ".bias", (48,))], 17)
    assert not head_fusable(sp0, sp3, "f16x3")
    ex = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3"))
    assert not ex.fuse_head(net.temp1)
    ex.record_variants = True
    x = torch.from_numpy(np.random.RandomState(40).standard_normal((T, 4, H, W)).astype(np.float32))
    oex = OracleExecutor(st, double=True)
    mid = ex.conv(sp0, x.to(_dev()), x_planar=True)
    assert ex.last_variant == "head_kernel<4>[f16x3 out]", ex.last_variant
    out = ex.conv(sp3, mid)
    assert ex.last_variant == NARROW, ex.last_variant
    want_mid = oex.conv(sp0, x, x_planar=True)
    assert mid.shape == (T, H, W, 48) and all(not h[..., 40:].any() for h in S.halves(mid.cpu()))
    got_mid = X3.from_split(mid.cpu())
    scale = max(1.0, float(want_mid.abs().max()))
    e0 = maxabs(got_mid.numpy(), want_mid.numpy())
    e1 = maxabs(X3.from_split(out.cpu()).numpy(), oex.conv(sp3, got_mid).numpy())
    e2 = maxabs(X3.from_split(out.cpu()).numpy(), oex.conv(sp3, want_mid).numpy())
    print("WIDTHS | entry | 4 -> 40 -> 48 unfused | head_kernel<4>[f16x3 out] + %s | max-abs: first conv %.3e, second %.3e, block %.3e" % (NARROW, e0, e1, e2))
    assert e0 < 2e-5 * scale and e1 < X3.TIGHT and e2 < X3.TIGHT      # (2e-5 x scale: the entry bound of test_gpu_f16x3's fused-entry test)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Winograd forms

WINO = [
    # cin, cout, tsm, act, epi, T, H, W      (H = 20 / 17: the last row band of the 16-row grid is the folded one)
    (384, 384, True, "relu6", 0, 3, 20, 19),        # fold 48; three 128-channel tiles (F(2,3)), six 64-channel ones (F(6,3))
    (128, 192, False, "relu", 0, 2, 9, 37),         # the second 128-channel tile of F(2,3) half live
    (144, 160, False, "none", 0, 1, 17, 33),        # 9 chunks; 160 = 128 + 32 and 2 x 64 + 32
    (128, 96, False, "relu6", 0, 2, 20, 24),        # one tile: 96 of 128, 64 + 32
    (128, 192, False, "none", 1, 1, 17, 21),        # PixelShuffle, Cout / 4 = 48
    (256, 384, False, "none", 1, 1, 12, 20),        # Cout / 4 = 96
]


@pytest.mark.parametrize("wide_conv", WN.PRODUCT_FORMS)
@pytest.mark.parametrize("cin,cout,tsm,act,epi,T,H,W", WINO)
def test_wino_layer_vs_oracle_and_model(wide_conv, cin, cout, tsm, act, epi, T, H, W):
    rows = WN.check_wino_layer(wide_conv, cin, cout, tsm, act, epi, T, H, W)      # (asserts winox_kernel<F(m,3) in last_variant per launch)
    assert len(rows) == (4 if tsm else 1) and all(("winox_kernel<F(%s,3)" % wide_conv[4]) in r[2] for r in rows)
    _table(wide_conv, rows)


@pytest.mark.parametrize("xf32", [False, True])
@pytest.mark.parametrize("wide_conv", WN.PRODUCT_FORMS)
@pytest.mark.parametrize("cin,cout,tsm,act,epi,T,H,W", WINO)
def test_wino_full_tile_and_folded_band_equal_the_half_height_tile(wide_conv, cin, cout, tsm, act, epi, T, H, W, xf32):
    """The grids of these cases are small, so the checker above ran the 8-row tile (wino_m 2 / 6: the kernel picks).  wino_m 42 / 46 never take
    it: the 16-row tile and, at H = 20 / 17 (F(2,3)), the folded last row band -- the same instruction sequence per output, so the same bits
    (test_gpu_wino.test_folded_last_row_band_is_bit_identical_to_the_half_height_tile), with fp16-pair and plain-fp32 tensors."""
    import ctypes
    from bsvd_amd import _lib
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    rs = np.random.RandomState(cin + cout + H + 2)
    m = int(wide_conv[4])
    sp = ConvSpec("l", "l", cin, cout, 1, tsm, act, epi)
    st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("l.weight", (cout, cin, 3, 3)),
                       ("l.bias", (cout,)), ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 7)
    gex = WN._exec(X3._Net(sp), st, wide_conv)
    gex.force_x_f32 = gex.force_y_f32 = xf32
    enc = (lambda t: t.to(_dev())) if xf32 else (lambda t: X3.to_split(t).to(_dev()))
    held = (lambda t: t) if xf32 else (lambda t: X3.from_split(X3.to_split(t)))      # the values the device tensor holds: what the oracle reads
    rnd = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))      # noqa: E731
    x_cpu = rnd(T, H, W, cin)
    skip_cpu, eps = (rnd(T, 2 * H, 2 * W, cout // 4), cout // 4) if epi == 1 else (None, 0)
    halos_cpu = [rnd(H, W, sp.fold), rnd(H, W, sp.fold)] if tsm else [None, None]
    x = enc(x_cpu)
    extra = None if skip_cpu is None else X3.to_split(skip_cpu).to(_dev())          # (the skip tensor stays an fp16-pair tensor)
    hp, hn = [None if h is None else Halo(enc(h), sp.fold, 0) for h in halos_cpu]
    ohp, ohn = [None if h is None else Halo(held(h), sp.fold, 0) for h in halos_cpu]
    want = OracleExecutor(st, double=True).conv(sp, held(x_cpu), ohp, ohn, None if skip_cpu is None else X3.from_split(X3.to_split(skip_cpu)), eps, 1)
    outs = {}
    for code in (m, 40 + m):
        a, y = gex.build_args(sp, x, hp, hn, extra, eps, 1)
        a.wino_m = code
        buf = ctypes.create_string_buffer(96)
        _lib.check(gex.lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96), "variant")
        _lib.check(gex.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "conv")
        torch.cuda.synchronize()
        outs[code] = (y, buf.value.decode())
    assert ("winox_kernel<F(%d,3)" % m) in outs[m][1] and "[8 rows]" in outs[m][1] and "[8 rows]" not in outs[40 + m][1], outs
    assert ("[f32 in]" in outs[40 + m][1]) == xf32
    assert torch.equal(outs[m][0], outs[40 + m][0])
    # ... and right on THESE operands (a fault both tiles share leaves them equal): the 16-row tile's result against the double-accumulating
    # oracle under the flat bound of test_gpu_wino / test_gpu_f32_handover
    y = outs[40 + m][0].cpu()
    err = maxabs((y if xf32 else X3.from_split(y)).numpy(), want.numpy())
    print("WIDTHS | %s | %s | f32 tensors %s | %s == %s bit for bit | max-abs %.3e" % (wide_conv, (cin, cout, tsm, act, epi, T, H, W), xf32,
                                                                                      outs[40 + m][1], outs[m][1], err))
    assert y.shape == want.shape and err < WN.TIGHT


@pytest.mark.parametrize("wide_conv", WN.PRODUCT_FORMS)
@pytest.mark.parametrize("cin,cout,tsm,act,epi,T,H,W", [WINO[0], WINO[4]])
def test_wino_layer_with_fp32_handover(wide_conv, cin, cout, tsm, act, epi, T, H, W):
    import test_gpu_f32_handover as FH
    FH.test_wino_layer_with_fp32_input_and_output_vs_oracle(wide_conv, cin, cout, tsm, act, epi, T, H, W)


def test_widths_the_kernels_do_not_serve_are_refused_with_their_code_and_launch_nothing():
    """the other side of the header's contract line on channel counts: -5 / -10 / -17 / -19 with the reason, y untouched; and the engine
    keeps a layer with Cout % 32 == 16 (or fold % 16 != 0) off the Winograd form"""
    import ctypes
    from bsvd_amd.engine import wino_eligible
    from bsvd_amd.netspec import ConvSpec
    st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("l.weight", (128, 128, 3, 3)),
                       ("l.bias", (128,)), ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 7)
    sp = ConvSpec("l", "l", 128, 128, 1, True, "relu6", 0)
    x = X3.to_split(torch.zeros(1, 8, 16, 128)).to(_dev())

    def refused(gex, code, what, **fields):
        a, y = gex.build_args(sp, x)
        for k, v in fields.items():
            setattr(a, k, v)
        y.fill_(12345.0)
        rc = gex.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        msg = gex.lib.bsvd_last_error().decode()
        assert rc == code and what in msg and bool((y == 12345.0).all()), (rc, msg, fields)

    direct = X3._exec(X3._Net(sp), st)
    refused(direct, -5, "multiples of 16", Cout=120)
    refused(direct, -5, "multiples of 16", Cin=40, fold=0)
    refused(direct, -10, "Cout % 64", Cout=96, fold=0, epilogue=1, act=0)
    refused(direct, -17, "fold", fold=24)                      # a 192-channel temporal-fusion layer
    refused(direct, -17, "fold", fold=8)                       # fold 8 is the 64-channel layers' alone
    for form in WN.PRODUCT_FORMS:
        wino = WN._exec(X3._Net(sp), st, form)
        refused(wino, -19, "multiple of 32", Cout=112)
        refused(wino, -19, "fold", fold=24)
    for cin, cout, tsm, ok in ((128, 112, False, False), (128, 80, False, False), (192, 192, True, False), (128, 96, False, True),
                               (144, 160, False, True), (384, 384, True, True)):
        assert wino_eligible(ConvSpec("l", "l", cin, cout, 1, tsm, "relu6", 0), "f16x3") == ok, (cin, cout, tsm)


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole networks

NETS = {
    "48-128-384": dict(chns=[48, 128, 384], mid_ch=40, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=40),
    "80-64-128": dict(chns=[80, 64, 128], mid_ch=48, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=70),
    "96-256-512": dict(chns=[96, 256, 512], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64),
    "blind 64-128-384": dict(chns=[64, 128, 384], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu", interm_ch=30, blind=True),
}
SIZES = [(3, 16, 24), (5, 20, 28)]
_CACHE = {}


def _model(name, st, precision):
    import bsvd_amd
    m = bsvd_amd.BSVD(pretrain_ckpt=None, precision=precision, **NETS[name])
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(_dev()).eval()


def _net_case(name, size):
    """per (network, size), computed once and left unchanged: weights, clip, the fp32 CPU oracle"""
    if (name, size) not in _CACHE:
        from oracle import bsvd_oracle as O
        c = NETS[name]
        blind = c.get("blind", False)
        st = seeded_state(bsvd_keys(c["chns"], c["mid_ch"], c["in_ch"], c["out_ch"], c["interm_ch"], blind), 23)
        T, H, W = size
        x = torch.from_numpy(np.random.RandomState(T + H).standard_normal((T, 3 if blind else 4, H, W)).astype(np.float32))
        cfg = O.default_cfg(chns=c["chns"], mid_ch=c["mid_ch"], act=c["act"], interm_ch=c["interm_ch"], blind=blind)
        _CACHE[(name, size)] = dict(st=st, x=x, want=O.bsvd_clip(x[None], O.to_torch_state(st), cfg)[0])
    return _CACHE[(name, size)]


def _per_frame(m, x):
    outs = [m.feedin_one_element(x[i:i + 1]) for i in range(x.shape[0])]
    while len(outs) < x.shape[0] + m.shift_num:
        outs.append(m.feedin_one_element(None))
    assert m.feedin_one_element(None) is None
    m.reset()
    return torch.cat(outs[m.shift_num:])


def _two_shards(name, st, precision, x):
    """the thread-halo helper of test_gpu_f16x3 / test_gpu_f16: two ranks on one device exchange compact halo slices through a barrier"""
    from bsvd_amd.dist import shard_range
    from bsvd_amd.schedule import Halo
    T = x.shape[0]
    world, boxes, results, errors = 2, {}, [None, None], []
    barrier = threading.Barrier(world)

    def rank(r):
        try:
            torch.cuda.set_device(0)
            m = _model(name, st, precision)
            ex = m._executor(_dev())

            class TH:
                def start(self, sp, v):
                    fold = sp.fold
                    boxes[(r, sp.key)] = (ex.halo_pack(v[0], 0, fold), ex.halo_pack(v[-1], fold, fold))

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

            a, b = shard_range(T, world, r)
            results[r] = m.clip_forward(x[a:b], TH())
            torch.cuda.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
            barrier.abort()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    return torch.cat(results)


def _clip(name, size, precision):
    """(model, its clip-schedule result), once per (network, size, precision)"""
    c = _net_case(name, size)
    if precision not in c:
        m = _model(name, c["st"], precision)
        assert m.precision == precision
        c[precision] = (m, m.clip_forward(c["x"].to(_dev())))
    return c[precision]


_IDS = ["%dx%dx%d" % s for s in SIZES]


@pytest.mark.parametrize("size", SIZES, ids=_IDS)
@pytest.mark.parametrize("name", list(NETS))
def test_network_clip_vs_oracle(name, size):
    """clip schedule against oracle.bsvd_oracle.bsvd_clip in fp32 and f16x3 under TOL = 1e-3 of test_gpu_f16x3 (the bar of
    test_gpu_fuzz.test_random_clip_whole_network); the exact-fp32 stream schedule bit-equal to its clip"""
    c = _net_case(name, size)
    errs = {}
    for precision in ("fp32", "f16x3"):
        m, clip = _clip(name, size, precision)
        errs[precision] = maxabs(clip.cpu().numpy(), c["want"].numpy())
        print("WIDTHS | net %s | T x H x W %s | %s | max-abs vs the fp32 CPU oracle %.3e (max |y| %.1f)"
              % (name, size, precision, errs[precision], float(c["want"].abs().max())))
    m, clip = _clip(name, size, "fp32")
    m.engine_mode = "stream"
    assert torch.equal(m(c["x"].to(_dev())[None])[0], clip)
    m.engine_mode = "clip"
    m.release_stream_buffers()
    assert errs["fp32"] < X3.TOL and errs["f16x3"] < X3.TOL, errs


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("size", SIZES, ids=_IDS)
@pytest.mark.parametrize("name", list(NETS))
def test_network_schedules_agree_bit_for_bit(name, size, precision):
    """per-frame feedin_one_element, streaming_forward at stream_chunk 1 / 3 / 'auto' with stream_overlap on and off, the graph-replayed
    second pass: all bit-equal to the clip schedule, within each split mode"""
    m, clip = _clip(name, size, precision)
    x = _net_case(name, size)["x"].to(_dev())
    for rep in range(2):              # the second pass replays the graphs the first one captured
        assert torch.equal(_per_frame(m, x), clip), ("per-frame stream", rep)
        for overlap in (True, False):
            m.stream_overlap = overlap
            for chunk in (1, 3, "auto"):
                m.stream_chunk = chunk
                assert torch.equal(m.streaming_forward(x), clip), ("chunked stream", chunk, overlap, rep)
        m.stream_overlap = True
    stt = m._stream_eng.stats
    assert stt["graph_captures"] > 0 and stt["graph_replays"] > 0, stt
    m.release_stream_buffers()


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("size", SIZES, ids=_IDS)
@pytest.mark.parametrize("name", list(NETS))
def test_network_two_shards_equal_the_whole_clip(name, size, precision):
    c = _net_case(name, size)
    assert torch.equal(_two_shards(name, c["st"], precision, c["x"].to(_dev())), _clip(name, size, precision)[1])


@pytest.mark.parametrize("size", SIZES, ids=_IDS)
@pytest.mark.parametrize("name", list(NETS))
def test_network_f16_error_within_twice_the_emulations(name, size):
    """test_gpu_f16.test_network_error_within_twice_the_emulations at these widths: max-abs against the double-accumulating oracle at most
    twice that of the CPU emulation of the mode (f16_model.F16EmuExecutor), computed here"""
    import f16_model as F
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import bsvd_clip
    c, n = _net_case(name, size), NETS[name]
    net = make_netspec(n["chns"], n["mid_ch"], n["in_ch"], n["out_ch"], n["act"], n["interm_ch"], blind=n.get("blind", False))
    w64 = bsvd_clip(OracleExecutor(c["st"], double=True), net, c["x"], x_planar=True, y_planar=(net.out_ch, None))
    emu = bsvd_clip(F.F16EmuExecutor(c["st"]), net, c["x"], x_planar=True, y_planar=(net.out_ch, None))
    e_emu = float((emu.double() - w64.double()).abs().max())
    e_gpu = float((_clip(name, size, "f16")[1].cpu().double() - w64.double()).abs().max())
    print("WIDTHS | net %s | T x H x W %s | f16 | max-abs vs the double-accumulating oracle executor: emulation %.3e, MI355X %.3e (%.2f x)" % (name, size, e_emu, e_gpu, e_gpu / e_emu))
    assert e_emu > 1e-5 and e_gpu <= 2 * e_emu, (name, size, e_gpu, e_emu)
