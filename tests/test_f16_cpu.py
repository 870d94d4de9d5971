"""precision='f16' (ABI BSVD_F16: one fp16 MFMA pass on the split16 layout) -- everything that needs no GPU.

  * the model of the mode (tests/f16_model.py) differs from the three-pass model by far more than the bound the GPU tests assert with, so
    those tests can tell the two modes apart; it reads no `lo` half of an activation, a halo or a weight
  * arch.BSVD accepts the mode, names it, refuses the three option pairs that need an 'f16x3'-only kernel, and 'auto' never resolves to it
  * the host schedules issue BSVD_F16 for exactly the MFMA layers, on BSVD_F16X3 packs
  * the library (loaded on the CPU like tests/test_abi.py does): the dtype is accepted, its refusals carry their own code and name the
    option, bsvd_conv3x3_variant says [f16]
"""
import ctypes

import numpy as np
import pytest
import torch

import f16_model as F
import split_model as S
from helpers import bsvd_keys
from seeded import seeded_clip, seeded_state

# name: (cin, cout, stride, tsm, act, epi, T, H, W)
LAYERS = {
    "64-64": (64, 64, 1, False, "relu6", 0, 1, 9, 12),
    "fold8 64-64": (64, 64, 1, True, "relu6", 0, 2, 6, 9),
    "128-128 fold16": (128, 128, 1, True, "relu6", 0, 2, 5, 9),
    "64-128 stride 2": (64, 128, 2, False, "relu6", 0, 1, 10, 12),
    "128-256 ps_add": (128, 256, 1, False, "none", 1, 1, 5, 6),
    "planar exit 64-3 resid": (64, 3, 1, False, "none", 2, 1, 8, 10),
}


def _operands(name, seed):
    from bsvd_amd.netspec import ConvSpec
    cin, cout, stride, tsm, act, epi, T, H, W = LAYERS[name]
    rs = np.random.RandomState(1000 * seed + cin + cout + H)
    sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
    w = (rs.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
    b = (rs.standard_normal(cout) * 0.1).astype(np.float32)
    xh, xl = S.pairs(rs.standard_normal((T, H, W, cin)).astype(np.float32))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw = {}
    if epi == 1:
        kw = dict(extra=sum(S.pairs(rs.standard_normal((T, 2 * Ho, 2 * Wo, cout // 4)).astype(np.float32))), extra_pstride=cout // 4, extra_cstride=1)
    elif epi == 2:
        kw = dict(extra=rs.standard_normal((T, 4, Ho, Wo)).astype(np.float32), extra_pstride=1, extra_cstride=Ho * Wo, y_planar=(3, None))
    return sp, rs, w, b, xh, xl, kw


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", list(LAYERS))
def test_one_pass_model_is_far_from_the_three_pass_model(name, seed):
    """|one pass - three passes| exceeds 10 x the GPU tests' bound (split_model.bound with M_DIRECT around the one-pass model): a kernel that
    ran three passes under dtype BSVD_F16 -- or one pass under BSVD_F16X3 -- cannot pass either mode's test"""
    sp, rs, w, b, xh, xl, kw = _operands(name, seed)
    one = F.direct_one_pass(sp, xh, xl, w, b, **kw)
    three = S.direct_three_pass(sp, xh, xl, w, b, **kw)
    err = S.chain_err(sp, xh + xl, w, b, **kw)
    ex = S.excess(three, one, err, F.M_DIRECT)
    print("%s seed %d: |three - one| = %.1f x the bound (chain err %.2e)" % (name, seed, ex, err))
    assert ex > 10.0, (name, seed, ex)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,tsm,epi,T,H,W", [(128, 128, True, 0, 2, 5, 9), (128, 256, False, 1, 1, 4, 6)])
def test_wino_one_pass_model_is_far_from_the_three_pass_model(cin, cout, tsm, epi, T, H, W, seed):
    from bsvd_amd.netspec import ConvSpec
    rs = np.random.RandomState(77 * seed + cin + cout)
    sp = ConvSpec("l", "l", cin, cout, 1, tsm, "none" if epi else "relu6", epi)
    w = S.detie_wino_weights((rs.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32), 2)
    b = (rs.standard_normal(cout) * 0.1).astype(np.float32)
    x = sum(S.pairs(rs.standard_normal((T, H, W, cin)).astype(np.float32)))
    kw = {}
    if epi == 1:
        kw = dict(extra=sum(S.pairs(rs.standard_normal((T, 2 * H, 2 * W, cout // 4)).astype(np.float32))), extra_pstride=cout // 4, extra_cstride=1)
    one = F.wino_one_pass(sp, x, w, 2, b, **kw)
    three = S.wino_model(sp, x, w, 2, b, **kw)
    err = S.wino_err(sp, x, w, 2, b, **kw)
    ex = S.excess(three, one, err, F.M_WINO2)
    print("wino2 %d-%d seed %d: |three - one| = %.1f x the bound" % (cin, cout, seed, ex))
    assert ex > 10.0, ex


@pytest.mark.parametrize("name", list(LAYERS))
def test_one_pass_model_reads_no_lo_half(name):
    from bsvd_amd.schedule import Halo
    sp, rs, w, b, xh, xl, kw = _operands(name, 5)
    T, H, W, cin = xh.shape
    hp = hn = hp2 = hn2 = None
    if sp.tsm:
        f = sp.fold
        ph, pl = S.pairs(rs.standard_normal((H, W, f)).astype(np.float32))
        nh, nl = S.pairs(rs.standard_normal((H, W, f)).astype(np.float32))
        hp, hn = (Halo(ph, f, 0), Halo(pl, f, 0)), (Halo(nh, f, 0), Halo(nl, f, 0))
        junk = S.fp16(rs.standard_normal((H, W, f)) * 100)
        hp2, hn2 = (Halo(ph, f, 0), Halo(junk, f, 0)), (Halo(nh, f, 0), Halo(-junk, f, 0))
    ref = F.direct_one_pass(sp, xh, xl, w, b, hp, hn, **kw)
    wh, wl = S.pairs(w)
    other = F.direct_one_pass(sp, xh, S.fp16(rs.standard_normal(xh.shape) * 100), w, b, hp2, hn2, w_pairs=(wh, S.fp16(rs.standard_normal(w.shape))), **kw)
    assert torch.equal(ref, other)
    # ... and it IS the three-pass model with those halves at zero
    z = lambda h: None if h is None else (h[0], Halo(np.zeros_like(S._np(h[1].t)), h[1].pstride, h[1].coff))
    three = S.direct_three_pass(sp, xh, np.zeros_like(xl), w, b, z(hp), z(hn), w_pairs=(wh, np.zeros_like(wl)), **kw)
    assert torch.equal(ref, three)
    assert float((ref - S.direct_three_pass(sp, xh, xl, w, b, hp, hn, **kw)).abs().max()) > 0


def test_wino_one_pass_model_reads_no_lo_of_the_transformed_pairs():
    from bsvd_amd.netspec import ConvSpec
    rs = np.random.RandomState(3)
    sp = ConvSpec("l", "l", 128, 128, 1, False, "relu6", 0)
    w = (rs.standard_normal((128, 128, 3, 3)) * 0.03).astype(np.float32)
    x = rs.standard_normal((1, 4, 6, 128)).astype(np.float32)
    U = np.einsum("xk,ocyk->xocy", S.WINO[2]["G"], w.astype(np.float64))
    uh, ul = S.pairs(U)
    a = F._wino_one_pass_pre(sp, x, w, 2)
    assert np.array_equal(a, F._wino_one_pass_pre(sp, x, w, 2, u_pairs=(uh, ul * 0 + 1.0)))
    # the INPUT's own lo halves do count (the kernel decodes hi + lo before it transforms): a different decoded value, a different result
    assert not np.array_equal(a, F._wino_one_pass_pre(sp, S.pairs(x)[0], w, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# arch.BSVD

KW = dict(chns=[32, 64, 128], mid_ch=32, norm="none", interm_ch=32, act="relu6", pretrain_ckpt=None)


def test_bsvd_accepts_and_names_the_mode():
    import bsvd_amd
    m = bsvd_amd.BSVD(precision="f16", **KW)
    assert m.precision == "f16" and m.precision_requested == "f16"
    assert "precision=f16" in m.extra_repr() and "ONE fp16 MFMA pass" in m.extra_repr() and "fp16-class" in m.extra_repr()
    assert "ONE fp16 MFMA pass" in repr(m)
    assert "'f16'" in bsvd_amd.BSVD.__doc__ and "fp16-CLASS" in bsvd_amd.BSVD.__doc__
    # same network requirements as 'f16x3'
    with pytest.raises(ValueError, match="precision='f16' needs temporal-fusion"):
        bsvd_amd.BSVD(precision="f16", chns=[48, 96, 200], mid_ch=48, norm="none", interm_ch=48, pretrain_ckpt=None)
    with pytest.raises(ValueError, match="precision must be"):
        bsvd_amd.BSVD(precision="fp16", **KW)


@pytest.mark.parametrize("kw,names", [(dict(wide_conv="wino6"), ("f16", "wide_conv='wino6'")), (dict(wide_conv="wino26"), ("f16", "wide_conv='wino26'")),
                                      (dict(v_handover=True), ("f16", "v_handover=True")), (dict(fuse_pairs=True), ("f16", "fuse_pairs=True"))])
def test_refused_option_pairs_raise_and_name_the_pair(kw, names):
    import bsvd_amd
    with pytest.raises(ValueError) as e:
        bsvd_amd.BSVD(precision="f16", **dict(KW, **kw))
    assert all(n in str(e.value) for n in names), str(e.value)
    # the same through the property setter on a model that was built with the option
    m = bsvd_amd.BSVD(precision="f16x3", **dict(KW, **kw))
    with pytest.raises(ValueError):
        m.precision = "f16"
    assert m.precision == "f16x3"
    bsvd_amd.BSVD(precision="f16", **dict(KW, wide_conv="direct"))
    bsvd_amd.BSVD(precision="f16", **dict(KW, wide_conv="wino2", v_handover=False, fuse_pairs=False))


def test_auto_never_yields_f16():
    import bsvd_amd
    for kw in (KW, dict(chns=[64, 128, 256], mid_ch=64, norm="none", interm_ch=64, act="relu6", pretrain_ckpt=None),
               dict(chns=[64, 128, 256], mid_ch=64, norm="none", interm_ch=30, act="relu", blind=True, pretrain_ckpt=None),
               dict(chns=[48, 96, 200], mid_ch=48, norm="none", interm_ch=48, pretrain_ckpt=None)):
        m = bsvd_amd.BSVD(precision="auto", **kw)
        assert m.precision in ("f16x3", "fp32")
        m.precision = "auto"
        assert m.precision in ("f16x3", "fp32")
    t = bsvd_amd.TSN(precision="f16", net2d_opt=dict(chns=[32, 64, 128], mid_ch=32, norm="none", interm_ch=32, act="relu6"), pretrain_ckpt=None)
    assert t.precision == "f16"
    t.precision = "auto"
    assert t.precision in ("f16x3", "fp32")


def test_precision_assignment_repacks(monkeypatch):
    """model.precision = 'f16' after construction: the next executor request packs again, in the new mode (F16X3 packs, BSVD_F16 launches)"""
    import bsvd_amd
    from bsvd_amd import engine
    packs = []

    class FakePacked:
        def __init__(self, net, state, device, precision, wide_conv, **kw):
            packs.append((precision, wide_conv, kw))
            self.precision, self.device = precision, device

    class FakeExec:
        def __init__(self, packed):
            self.packed = packed

    monkeypatch.setattr(engine, "require_hip", lambda: None)
    monkeypatch.setattr(engine, "PackedNet", FakePacked)
    monkeypatch.setattr(engine, "HipExecutor", FakeExec)
    m = bsvd_amd.BSVD(precision="f16x3", **KW)
    e1 = m._executor("cpu")
    assert m._executor("cpu") is e1 and len(packs) == 1
    m.precision = "f16"
    e2 = m._executor("cpu")
    assert e2 is not e1 and [p[0] for p in packs] == ["f16x3", "f16"] and m.precision == "f16"
    m.wide_conv = "wino6"           # a plain attribute: caught at the next pack
    with pytest.raises(ValueError, match="wino6"):
        m._executor("cpu")


# ---------------------------------------------------------------------------------------------------------------------------------------
# host schedules: what would be issued

class _IssueLog(F.F16EmuExecutor):
    """the oracle-backed executor, logging per launch the BsvdConvArgs.dtype and the pack dtype engine.py decides for precision='f16'"""

    def __init__(self, st, net, fuse_head):
        super().__init__(st)
        self.net, self.fuse = net, fuse_head
        self.launch_log = []

    def _log(self, sp, x_planar, head):
        """what HipExecutor.build_args decides from the arguments the SCHEDULE passed (engine.is_mfma_launch is its predicate), and what
        PackedNet packs for the layer (its `edge` set: the first layer of the network)"""
        from bsvd_amd import engine
        mfma = engine.is_mfma_launch(x_planar, head)
        self.launch_log.append((sp.key, mfma, engine.launch_dtype("f16", mfma), engine.pack_dtype("f16", sp.key == self.net.layers[0].key)))

    def fuse_head(self, S_):
        from bsvd_amd.engine import head_fusable
        return bool(self.fuse and "inc0" in S_ and S_["inc0"] is self.net.layers[0] and head_fusable(S_["inc0"], S_["inc3"], "f16"))

    def conv_head_fused(self, sp0, sp3, x, out=None):
        n = len(self.launch_log)
        y = self.conv(sp3, self.conv(sp0, x, x_planar=True))
        del self.launch_log[n:]
        self._log(sp3, True, sp0)              # one launch, keyed by the second conv, on planar input with the first conv as `head`
        if out is not None:
            out.copy_(y)
            return out
        return y

    def conv(self, sp, x, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, x_planar=False, y_planar=None, out=None):
        if out is None:
            self._log(sp, x_planar, None)
        return super().conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar, out)


@pytest.mark.parametrize("fuse_head", [True, False])
@pytest.mark.parametrize("schedule", ["clip", "stream"])
def test_host_schedules_issue_f16_for_exactly_the_mfma_layers(schedule, fuse_head):
    from bsvd_amd import _lib
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import StreamPipeline, bsvd_clip
    chns = [32, 64, 128]
    st = seeded_state(bsvd_keys(chns, 32, 4, 3, 32), 3)
    net = make_netspec(chns, 32, 4, 3, "relu6", 32)
    ex = _IssueLog(st, net, fuse_head)
    x = torch.from_numpy(seeded_clip((1, 3, 4, 8, 12), 4, kind="sigma30"))[0]
    if schedule == "clip":
        bsvd_clip(ex, net, x, x_planar=True, y_planar=(net.out_ch, None))
    else:
        pipe = StreamPipeline(net)
        for t in list(range(x.shape[0])) + [None] * (pipe.shift_num + 1):
            pipe.feed(ex, None if t is None else x[t:t + 1], x_planar=True, y_planar=(net.out_ch, None))
    first = net.layers[0].key
    assert ex.launch_log
    for key, mfma, dt, pk in ex.launch_log:
        if key == first:
            assert not fuse_head and not mfma and dt == _lib.BSVD_F16X3 and pk == _lib.BSVD_F32       # the fp32 head kernel, an fp32 pack
        else:
            assert mfma and dt == _lib.BSVD_F16 and pk == _lib.BSVD_F16X3, (key, dt, pk)
    keys = {k for k, *_ in ex.launch_log}
    assert keys == {sp.key for sp in net.layers} - ({first} if fuse_head else set())
    assert _lib.BSVD_F16 == 3 and _lib.BSVD_F16X3 == 2 and _lib.BSVD_F32 == 0


def test_engine_mode_predicates():
    from bsvd_amd import arch, engine
    from bsvd_amd.netspec import ConvSpec, make_netspec
    assert arch.SPLIT_PRECISIONS is engine.SPLIT_PRECISIONS
    assert engine.is_mfma_launch(False, None) and engine.is_mfma_launch(True, object()) and not engine.is_mfma_launch(True, None)
    # pair_fusable is what it was for 'f16x3': plain stride-1 convs only -- no temporal shift, no PixelShuffle first conv, no stride 2
    mk = lambda cin, cout, stride=1, tsm=False, epi=0: ConvSpec("l", "l", cin, cout, stride, tsm, "relu6", epi)
    assert engine.pair_fusable(mk(64, 64), mk(64, 64), "f16x3") and engine.pair_fusable(mk(64, 64), mk(64, 3, epi=2), "f16x3")
    assert not engine.pair_fusable(mk(64, 64, tsm=True), mk(64, 64), "f16x3") and not engine.pair_fusable(mk(64, 64), mk(64, 64, tsm=True), "f16x3")
    assert not engine.pair_fusable(mk(64, 256, epi=1), mk(64, 64), "f16x3") and not engine.pair_fusable(mk(64, 64), mk(64, 256, epi=1), "f16x3")
    assert not engine.pair_fusable(mk(64, 64, stride=2), mk(64, 64), "f16x3") and not engine.pair_fusable(mk(64, 64), mk(64, 64), "fp32")
    net = make_netspec([64, 128, 256], 64, 4, 3, "relu6", 64)
    t1 = net.temp1
    assert engine.head_fusable(t1["inc0"], t1["inc3"], "f16") and engine.head_fusable(t1["inc0"], t1["inc3"], "f16x3")
    assert engine.pair_fusable(t1["out0"], t1["out3"], "f16x3") and not engine.pair_fusable(t1["out0"], t1["out3"], "f16")
    wide = [sp for sp in net.layers if engine.wino_eligible(sp, "f16x3")]
    assert wide and wide == [sp for sp in net.layers if engine.wino_eligible(sp, "f16")]
    assert not any(engine.wino_eligible(sp, "fp32") for sp in net.layers)
    assert engine.launch_dtype("fp32") == 0 and engine.launch_dtype("f16x3") == 2 and engine.launch_dtype("f16x3", False) == 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# the library, loaded on the CPU

def _variant(lib, **kw):
    from bsvd_amd import _lib
    buf = ctypes.create_string_buffer(96)
    a = _lib.BsvdConvArgs()
    a.x = a.y = a.w_packed = 256
    a.frames, a.H, a.W, a.Cin, a.Cout, a.stride, a.dtype = 10, 270, 480, 128, 128, 1, _lib.BSVD_F16
    for k, v in kw.items():
        setattr(a, k, v)
    rc = lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96)
    return rc, buf.value.decode(), lib.bsvd_last_error().decode() if rc < 0 else ""


def test_library_accepts_the_dtype_and_names_its_kernels():
    from bsvd_amd import _lib
    lib = _lib.load()
    assert lib.bsvd_abi_version() == _lib.ABI_VERSION and lib.bsvd_conv_args_size() == ctypes.sizeof(_lib.BsvdConvArgs)
    v = lambda **kw: _variant(lib, **kw)[:2]
    # every direct-form split tile launch_conv3x3 selects: [f16] where BSVD_F16X3 says [f16x3]
    for kw, name in ((dict(), "conv3x3_kernel<4,2,2,2,1>[%s]"), (dict(frames=1), "conv3x3_kernel<2,2,2,2,1>[%s]"),
                     (dict(Cin=64, Cout=64), "conv3x3_kernel<4,1,2,2,1>[%s]"), (dict(Cin=64, Cout=64, fold=8), "conv3x3_kernel<2,2,4,1,1>[%s][fold8]"),
                     (dict(Cin=64, Cout=16, y_planar_ch=3, epilogue=2, extra=256, resid_ch=3), "conv3x3_kernel<2,1,4,1,1>[%s][planar out]"),
                     (dict(Cin=64, stride=2), "conv3x3_kernel<4,1,1,4,2>[%s]"),
                     (dict(Cin=64, Cout=64, x_planar_ch=4, head_w_packed=256, head_bias=256), "conv3x3_kernel<4,1,2,2,1>[%s][fused entry]"),
                     (dict(w_wino_packed=256, wino_m=2, H=135, W=240, Cin=256, Cout=256), "winox_kernel<F(2,3),2x2>[%s]"),
                     (dict(w_wino_packed=256, wino_m=2, H=135, W=240, frames=1), "winox_kernel<F(2,3),2x2>[%s][8 rows]"),
                     (dict(w_wino_packed=256, wino_m=42, H=135, W=240, frames=1), "winox_kernel<F(2,3),2x2>[%s]"),
                     (dict(w_wino_packed=256, wino_m=2, x_f32=1, y_f32=1), "winox_kernel<F(2,3),2x2>[%s][f32 in]"),
                     (dict(w_wino_packed=256, wino_m=2, Cout=256, epilogue=1), "winox_kernel<F(2,3),2x2>[%s]")):
        assert v(**kw) == (0, name % "f16"), (kw, v(**kw))
        assert v(dtype=_lib.BSVD_F16X3, **kw) == (0, name % "f16x3"), kw
    # the weight scale is an option of both split modes
    assert v(out_scale=0.5)[0] == 0 and v(Cin=64, Cout=64, x_planar_ch=4, head_w_packed=256, head_bias=256, head_out_scale=2.0)[0] == 0
    # the retired value 1 stays refused, like every unknown dtype
    assert v(dtype=1)[0] == -2 and v(dtype=7)[0] == -2


def test_library_refusals_have_their_own_code_and_name_the_option():
    from bsvd_amd import _lib
    lib = _lib.load()
    r = lambda **kw: _variant(lib, **kw)
    rc, _, msg = r(Cin=64, Cout=64, pre_w_packed=256, pre_bias=256, pre_cin=64)
    assert rc == -24 and "BSVD_F16" in msg and "pre_w_packed" in msg
    rc, _, msg = r(w_wino_packed=256, wino_m=6, Cin=256, Cout=256)
    assert rc == -24 and "wino_m 6" in msg
    assert r(w_wino_packed=256, wino_m=46, Cin=256, Cout=256)[0] == -24
    rc, _, msg = r(w_wino_packed=256, wino_m=2, x_v=2)
    assert rc == -24 and "x_v" in msg
    rc, _, msg = r(w_wino_packed=256, wino_m=2, y_v=2)
    assert rc == -24 and "y_v" in msg
    rc, _, msg = r(Cin=16, Cout=64, x_planar_ch=4)
    assert rc == -24 and "x_planar_ch" in msg
    # the BSVD_F16X3 refusals apply unchanged: alignment, fold, 2 GiB
    assert r(fold=12)[0] == -17 and "fold 12" in r(fold=12)[2]
    assert r(x=260)[0] == -17
    rc, _, msg = r(frames=1, H=4320, W=7680, Cin=64, Cout=64)
    assert rc == -17 and "2 GiB" in msg
    assert r(stride=2, Cin=64, fold=16)[0] == -17
    # no BSVD_F16 pack: an F16X3 pack serves both modes
    assert lib.bsvd_pack_weights(16, None, 16, 16, 16, 16, 0, _lib.BSVD_F16, 16, 16, None) == -2
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "bsvd_hip.h")).read()
    assert "serves BOTH modes" in hdr and "reserved and not implemented" not in hdr and "BSVD_F16 = 3" in hdr
