"""The conv kernels and the layout helpers on tensors that are NOT tight and NOT alone (include/bsvd_hip.h, Conventions: every stride is the
caller's): frames a slack apart, halos and the epilogue's second operand inside wider holding tensors, everything inside arenas of the test's
own (tests/arena.py) whose slack, guards and foreign channels are NaN.  engine.build_args only ever writes H*W*C into a stride field, so
without these cases one H*W*C in the place of x_fs / y_fs / extra_fs in a kernel -- or a store outside y, a value from outside a tensor that
reaches a result, an element of y nobody writes -- passes the whole suite.

Every case: one tight launch, then the same args re-homed into arenas (arena.rehome), launched on a 0x00 and on a 0xFF pre-filled output
arena.  Asserted (arena.verdict): both pre-fills give the same bits; the bits of the tight launch where bsvd_conv3x3_variant names the same
instantiation; the existing bound against OracleExecutor(double=True) on the logical operands (TOL of test_gpu_parity, TIGHT of
test_gpu_f16x3 / test_gpu_wino -- imported, none invented here); no NaN; no byte of any arena outside its logical elements changed; the
variant name carries what the case declares.

Layouts: A frame slack 20 on x, y, extra (80 bytes: a multiple of 16, not of 64); B halos inside Cin + 16 channel holding tensors at coff
16 + fold / 16 ("b": compact slices inside fold + 16 channels at coff 16; "F": a neighbour frame behind 16 foreign channels, the form a
fold-8 half chunk of fp16 pairs has); C the epilogue's second operand inside a 16 channels wider holding tensor; D frame slack 5 on x -- the
exact-fp32 mode runs its [generic] kernel, the split mode and the Winograd form refuse with a reason and write nothing.  ("d": the fused entry
reads a planar fp32 input with scalar loads and has no alignment to lose: it runs, on the same instantiation.)

What this does not see: a load from outside a tensor whose value a select discards (value poisoning cannot), and offsets near 2 GiB."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena
from oracle_exec import OracleExecutor
from seeded import seeded_state
from test_gpu_f16x3 import TIGHT, _Net, from_split, to_split
from test_gpu_f16x3 import _exec as _split_exec
from test_gpu_pair import _setup as _pair_setup
from test_gpu_parity import TOL, _gpu_exec, _one_layer_net
from test_gpu_v_handover import _layer as _v_layer
from test_gpu_v_handover import _to_v
from test_gpu_wino import TIGHT as WINO_TIGHT
from test_gpu_wino import _exec as _wino_exec

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _ident(t):
    return t


def _quant(t):
    return from_split(to_split(t))


def _state3(cin, cout, seed=7):
    return seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,)),
                         ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], seed)


def _storage(v):
    """the torch tensor behind an activation: itself, or the [T, frame elems] storage of a transformed-domain tensor"""
    from bsvd_amd.engine import VT
    return v.t if isinstance(v, VT) else v


def _variant(lib, a):
    buf = ctypes.create_string_buffer(128)
    rc = lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 128)
    return rc, buf.value.decode()


def _go(lib, a):
    rc = lib.bsvd_conv3x3(ctypes.byref(a), _stream())
    assert rc == 0, (rc, lib.bsvd_last_error())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the families
# A family = one executor, its logical operands and ONE reference, shared by all its layouts (functools.lru_cache).  Fields: ex, sp, x (device
# tensor as the engine holds it), kw (build_args keywords: device halos, extra, ...), tweak(args), expect (variant substring), ref, tol, decode.

def _args(c):
    a, y = c.ex.build_args(c.sp, c.x, **c.kw)
    c.tweak(a)
    return a, y


def _no_tweak(a):
    pass


_REFS = {}


@functools.lru_cache(maxsize=None)
def _layer(prec, cin, cout, stride, tsm, act, epi, T, H, W, halos="none", extra="none", y_planar=None, wide_conv="direct", code=0, fat=0,
           xf32=False, yf32=False):
    """one NHWC layer as test_gpu_parity / test_gpu_f16x3 / test_gpu_wino / test_gpu_f32_handover set it up"""
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    rs = np.random.RandomState(cin * 1000 + cout + stride + H)
    if prec == "f32":
        st = seeded_state([("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,))], 7)
        net, sp = _one_layer_net(cin, cout, stride, tsm, act, epi)
        ex, tol = _gpu_exec(net, st), TOL
    else:
        sp, st = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi), _state3(cin, cout)
        ex = _split_exec(_Net(sp), st) if wide_conv == "direct" else _wino_exec(_Net(sp), st, wide_conv)
        tol = TIGHT if wide_conv == "direct" else WINO_TIGHT
        assert ("l" in ex.packed.wino) == (wide_conv != "direct")
        ex.force_x_f32, ex.force_y_f32 = xf32, yf32
    split = prec != "f32"
    enc_x, q_x = (to_split, _quant) if split and not xf32 else (_ident, _ident)      # x and its halos: fp16 pairs unless handed over as fp32
    enc_e, q_e = (to_split, _quant) if split else (_ident, _ident)                  # NHWC second operands of the epilogue: always the engine's tensors
    decode = from_split if split and not yf32 and y_planar is None else None
    oex = OracleExecutor(st, double=True)
    x = q_x(_randn(rs, T, H, W, cin))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw, okw = {}, {}
    if extra == "ps":                   # PixelShuffle skip tensor, laid out like y
        e = q_e(_randn(rs, T, 2 * Ho, 2 * Wo, cout // 4))
        kw.update(extra=enc_e(e).to(_dev()), extra_pstride=cout // 4, extra_cstride=1)
        okw.update(extra=e, extra_pstride=cout // 4, extra_cstride=1)
    elif extra == "nhwc64":             # residual base: an fp32 NHWC tensor (pstride 64, cstride 1)
        e = _randn(rs, T, Ho, Wo, 64)
        kw.update(extra=e.to(_dev()), extra_pstride=64, extra_cstride=1)
        okw.update(extra=e, extra_pstride=64, extra_cstride=1)
    elif extra == "planar4":            # ... the planar network input (1, H*W)
        e = _randn(rs, T, 4, Ho, Wo)
        kw.update(extra=e.to(_dev()), extra_pstride=1, extra_cstride=Ho * Wo)
        okw.update(extra=e, extra_pstride=1, extra_cstride=Ho * Wo)
    elif extra == "split64":            # ... a split16 engine tensor (BsvdConvArgs.extra_split)
        e = _quant(_randn(rs, T, Ho, Wo, 64))
        kw.update(extra=to_split(e).to(_dev()), extra_pstride=64, extra_cstride=1)
        okw.update(extra=e, extra_pstride=64, extra_cstride=1)
    if halos != "none":
        fold = sp.fold
        if halos == "compact":
            hp, hn = Halo(q_x(_randn(rs, H, W, fold)), fold, 0), Halo(q_x(_randn(rs, H, W, fold)), fold, 0)
        else:
            full = q_x(_randn(rs, 1, H, W, cin))
            hp, hn = Halo(full, cin, fold), Halo(full, cin, 0)
        kw.update(halo_prev=Halo(enc_x(hp.t).to(_dev()), hp.pstride, hp.coff), halo_next=Halo(enc_x(hn.t).to(_dev()), hn.pstride, hn.coff))
        okw.update(halo_prev=hp, halo_next=hn)
    if y_planar is not None:
        kw.update(y_planar=y_planar)
        okw.update(y_planar=y_planar)
    # the operands depend on neither the form nor its code: F(2,3), F(6,3) and their codes share one reference
    key = (prec, cin, cout, stride, tsm, act, epi, T, H, W, halos, extra, y_planar, xf32)
    if key not in _REFS:
        _REFS[key] = oex.conv(sp, x, **okw)
    ref = _REFS[key]

    def tweak(a):
        if code:
            a.wino_m = code
        if fat:
            a.fat_min_wgs = fat
    return SimpleNamespace(ex=ex, sp=sp, x=enc_x(x).to(_dev()), kw=kw, tweak=tweak, ref=ref, tol=tol, decode=decode)


@functools.lru_cache(maxsize=None)
def _head(cin, cout, act, T, H, W):
    """the exact-fp32 planar entry layer (test_gpu_parity.test_edge_layers_vs_oracle)"""
    rs = np.random.RandomState(cin * 100 + cout + H)
    st = seeded_state([("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,))], 9)
    net, sp = _one_layer_net(cin, cout, 1, False, act, 0)
    x = _randn(rs, T, cin, H, W)
    return SimpleNamespace(ex=_gpu_exec(net, st), sp=sp, x=x.to(_dev()), kw=dict(x_planar=True), tweak=_no_tweak,
                           ref=OracleExecutor(st, double=True).conv(sp, x, x_planar=True), tol=TOL, decode=None)


@functools.lru_cache(maxsize=None)
def _entry(cin, cmid, cout, act, T, H, W):
    """InputCvBlock in one launch (test_gpu_f16x3.test_fused_entry_vs_two_step_oracle_and_vs_the_unfused_kernels)"""
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import ConvSpec
    sp0 = ConvSpec("inc0", "b.inc.convblock.0", cin, cmid, 1, False, act, 0)
    sp3 = ConvSpec("inc3", "b.inc.convblock.3", cmid, cout, 1, False, act, 0)
    net = SimpleNamespace(layers=[sp0, sp3], temp1={"inc0": sp0, "inc3": sp3})
    st = seeded_state([(sp0.key + ".weight", (cmid, cin, 3, 3)), (sp0.key + ".bias", (cmid,)),
                       (sp3.key + ".weight", (cout, cmid, 3, 3)), (sp3.key + ".bias", (cout,))], 17)
    rs = np.random.RandomState(cin + cmid + H)
    x = _randn(rs, T, cin, H, W)
    oex = OracleExecutor(st, double=True)
    ex = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3"))
    assert ex.fuse_head(net.temp1)
    return SimpleNamespace(ex=ex, sp=sp3, x=x.to(_dev()), kw=dict(x_planar=True, head=sp0), tweak=_no_tweak,
                           ref=oex.conv(sp3, oex.conv(sp0, x, x_planar=True)), tol=TIGHT, decode=from_split)


@functools.lru_cache(maxsize=None)
def _pair(cb, T, H, W):
    """the fused pair of test_gpu_pair: 64 -> 64 -> 64 PLAIN, or 64 -> 64 -> 3 with the planar RESID exit (split16 base, clamp)"""
    a, b, st, fused, _ = _pair_setup(64, 64, cb, "relu6", "relu6" if cb == 64 else "none", 0 if cb == 64 else 2)
    rs = np.random.RandomState(T * 100 + H + cb)
    x = _quant(torch.from_numpy((rs.rand(T, H, W, 64) * 3 - 0.5).astype(np.float32)))
    oex = OracleExecutor(st, double=True)
    mid = _quant(oex.conv(a, x).float())              # the tensor between the convs is carried as fp16 pairs
    kw, okw = dict(pre=a), {}
    if cb != 64:
        base = _quant(torch.from_numpy(rs.rand(T, H, W, 64).astype(np.float32)))
        okw = dict(extra=base, extra_pstride=64, extra_cstride=1, y_planar=(3, (0.0, 1.0)))
        kw.update(okw, extra=to_split(base).to(_dev()))
    return SimpleNamespace(ex=fused, sp=b, x=to_split(x).to(_dev()), kw=kw, tweak=_no_tweak, ref=oex.conv(b, mid, **okw), tol=TIGHT,
                           decode=from_split if cb == 64 else None)


S1, S3 = (1, 19, 21), (3, 19, 21)
# name: (builder, arguments, declared variant substring, layouts)
FAMILIES = {
    # ---- exact fp32
    "f32 narrow": (_layer, ("f32", 64, 64, 1, False, "relu6", 0) + S3, "<2,2,4,1,1>[f32]", "AD"),
    "f32 fold8": (_layer, ("f32", 64, 64, 1, True, "relu6", 0) + S3 + ("full",), "[fold8]", "ABbD"),
    "f32 wide": (_layer, ("f32", 128, 128, 1, True, "relu6", 0) + S3 + ("full",), "<2,2,2,2,1>[f32]", "ABbD"),
    "f32 wide, one frame": (_layer, ("f32", 128, 128, 1, True, "relu6", 0) + S1 + ("compact",), "<2,2,2,2,1>[f32]", "ABb"),
    "f32 stride 2": (_layer, ("f32", 64, 128, 2, False, "relu6", 0, 2, 21, 19), "<2,2,2,2,2>[f32]", "AD"),
    "f32 PS_ADD": (_layer, ("f32", 256, 512, 1, False, "none", 1, 2, 9, 13, "none", "ps"), "conv3x3_kernel<", "ACD"),
    "f32 RESID, NHWC base": (_layer, ("f32", 64, 64, 1, False, "none", 2, 2, 12, 20, "none", "nhwc64"), "conv3x3_kernel<", "ACD"),
    "f32 RESID, planar base": (_layer, ("f32", 64, 64, 1, False, "none", 2, 2, 12, 20, "none", "planar4"), "conv3x3_kernel<", "AD"),
    "f32 head 4": (_head, (4, 64, "relu6", 2, 21, 37), "head_kernel<4>", "AD"),
    "f32 head 3": (_head, (3, 30, "relu", 2, 21, 37), "head_kernel<3>", "AD"),
    "f32 tail 3, clamp": (_layer, ("f32", 64, 3, 1, False, "none", 2, 2, 21, 37, "none", "planar4", (3, (0.0, 1.0))), "tail_kernel<3>", "AD"),
    "f32 tail 3, NHWC base": (_layer, ("f32", 64, 3, 1, False, "none", 2, 2, 21, 37, "none", "nhwc64", (3, None)), "tail_kernel<3>", "AC"),
    "f32 tail 4": (_layer, ("f32", 64, 4, 1, False, "relu", 2, 2, 21, 37, "none", "planar4", (4, None)), "tail_kernel<4>", "AD"),
    # ---- split fp16, direct form
    "f16x3 narrow": (_layer, ("f16x3", 64, 64, 1, False, "relu6", 0) + S3, "<4,1,2,2,1>[f16x3]", "AD"),
    "f16x3 fold8, frames": (_layer, ("f16x3", 64, 64, 1, True, "relu6", 0) + S3 + ("full",), "<2,2,4,1,1>[f16x3][fold8]", "AFD"),
    "f16x3 fold8, slices": (_layer, ("f16x3", 64, 64, 1, True, "relu6", 0) + S1 + ("compact",), "<2,2,4,1,1>[f16x3][fold8]", "A"),
    "f16x3 wide": (_layer, ("f16x3", 128, 128, 1, True, "relu6", 0) + S3 + ("full",), "<2,2,2,2,1>[f16x3]", "ABbD"),
    "f16x3 fat": (_layer, ("f16x3", 128, 128, 1, True, "relu6", 0) + S3 + ("full", "none", None, "direct", 0, 1), "<4,2,2,2,1>[f16x3]", "ABb"),
    # (one frame of 5 rows: the lower wave pair of the only tile row lies below the image)
    "f16x3 fat, waves below the image": (_layer, ("f16x3", 128, 128, 1, True, "relu6", 0, 1, 5, 21, "compact", "none", None, "direct", 0, 1),
                                         "<4,2,2,2,1>[f16x3]", "AB"),
    "f16x3 stride 2": (_layer, ("f16x3", 64, 128, 2, False, "relu6", 0, 2, 21, 19), "<4,1,1,4,2>", "AD"),
    "f16x3 PS_ADD": (_layer, ("f16x3", 128, 256, 1, False, "none", 1, 2, 9, 13, "none", "ps"), "[f16x3]", "ACD"),
    "f16x3 exit": (_layer, ("f16x3", 64, 3, 1, False, "none", 2, 2, 21, 37, "none", "split64", (3, (0.0, 1.0))), "[planar out]", "ACD"),
    "f16x3 entry 4": (_entry, (4, 64, 64, "relu6", 2, 21, 37), "[fused entry]", "Ad"),
    "f16x3 entry 3": (_entry, (3, 32, 64, "relu", 2, 21, 37), "[fused entry]", "Ad"),
    "f16x3 pair": (_pair, (64, 2, 19, 21), "<4,1,2,2,1>[f16x3][fused pair]", "AD"),
    "f16x3 pair, exit": (_pair, (3, 2, 19, 21), "<2,1,4,1,1>[f16x3][planar out][fused pair]", "ACD"),
    # ---- split fp16, direct form, channel widths off the power-of-two grid (tests/test_gpu_widths.py): a masked-channel store behind the last
    #      pixel of a frame lands in the frame slack or the guard band here, nowhere else in the suite
    "f16x3 narrow, Cout 48": (_layer, ("f16x3", 48, 48, 1, False, "relu6", 0) + S3, "<4,1,2,2,1>[f16x3]", "AD"),
    "f16x3 wide, Cout 80": (_layer, ("f16x3", 80, 80, 1, False, "relu6", 0) + S3, "<2,2,2,2,1>[f16x3]", "AD"),
    "f16x3 fat, Cout 80": (_layer, ("f16x3", 80, 80, 1, False, "relu6", 0) + S3 + ("none", "none", None, "direct", 0, 1), "<4,2,2,2,1>[f16x3]", "A"),
    "f16x3 PS_ADD, Cout 192": (_layer, ("f16x3", 128, 192, 1, False, "none", 1, 2, 9, 13, "none", "ps"), "<2,2,2,2,1>[f16x3]", "ACD"),
    "f16x3 stride 2, 80 -> 64": (_layer, ("f16x3", 80, 64, 2, False, "relu6", 0, 2, 21, 19), "<4,1,1,4,2>", "AD"),
    # ---- plain-fp32 hand-over
    "f16x3 direct producer, y_f32": (_layer, ("f16x3", 128, 128, 1, False, "relu6", 0, 3, 19, 50, "none", "none", None, "direct", 0, 0, False, True),
                                     "[f16x3]", "A"),
}
# ---- Winograd form.  W = 50 crosses the 16-pixel F(2,3) tile and the 48-pixel F(6,3) tile; H = 19: a last row band of 3 rows (F(2,3): folded,
# F(6,3): on the 8-row body), H = 27: one of 11 rows; codes 42 / 46 never take the half-height tile, 2 / 6 take it for the one-frame grid.
# The full-tile cases declare that "[8 rows]" is ABSENT: a dispatch change cannot move them onto the half-height tile unnoticed.  The folded
# band is a launch-time choice inside the full-tile kernel that bsvd_conv3x3_variant does not name: H = 19 with the fixed codes is the
# size at which the library folds (tests/test_gpu_wino.py FOLD_CASES), no name can pin it.
for _m, _auto, _fixed in ((2, 2, 42), (6, 6, 46)):
    _w, _k = "wino%d" % _m, "winox_kernel<F(%d,3)" % _m
    _full = _k + "*![8 rows]"
    _tsm = ("f16x3", 128, 128, 1, True, "relu6", 0)
    FAMILIES.update({
        "F(%d,3) short band" % _m: (_layer, _tsm + (3, 19, 50, "full", "none", None, _w, _fixed), _full, "ABbD"),
        "F(%d,3) short band, half-height tile" % _m: (_layer, _tsm + (3, 19, 50, "full", "none", None, _w, _auto), _k + "*[8 rows]", "A"),
        "F(%d,3) long band" % _m: (_layer, _tsm + (3, 27, 50, "full", "none", None, _w, _fixed), _full, "AB"),
        "F(%d,3) one frame" % _m: (_layer, _tsm + (1, 19, 50, "compact", "none", None, _w, _auto), _k + "*[8 rows]", "ABb"),
        "F(%d,3) PS_ADD" % _m: (_layer, ("f16x3", 256, 512, 1, False, "none", 1, 2, 19, 50, "none", "ps", None, _w, _fixed), _full, "ACD"),
        "F(%d,3) PS_ADD one frame" % _m: (_layer, ("f16x3", 256, 512, 1, False, "none", 1, 1, 27, 50, "none", "ps", None, _w, _auto), _k, "AC"),
        "F(%d,3) f32 in" % _m: (_layer, _tsm + (3, 19, 50, "full", "none", None, _w, _fixed, 0, True, False), _full + "*[f32 in]", "ABD"),
        "F(%d,3) f32 in and out" % _m: (_layer, _tsm + (3, 19, 50, "full", "none", None, _w, _fixed, 0, True, True), _full + "*[f32 in]", "AB"),
        # (Cout 192: the second 128-channel tile of F(2,3) half live, three 64-channel tiles of F(6,3))
        "F(%d,3) Cout 192" % _m: (_layer, ("f16x3", 128, 192, 1, False, "relu6", 0, 3, 19, 50, "none", "none", None, _w, _fixed), _full, "AD"),
    })

LAYOUTS = {"A": {}, "B": dict(halo_layout="wide"), "b": dict(halo_layout="compact"), "F": dict(halo_layout="half"), "C": dict(widen_extra=16),
           "D": dict(x_slack=5), "d": dict(x_slack=5)}
CASES = [(f, lay) for f, (_, _, _, lays) in FAMILIES.items() for lay in lays]


def _declared(expect, name):
    """every piece of a declared 'a*b' substring list is in the name; a piece '!c' must NOT be in it"""
    return all((part[1:] not in name) if part.startswith("!") else (part in name) for part in expect.split("*"))


def _half_chunk_halo(t, cin, second):
    """The 8-channel half chunk of fp16 pairs a fold-8 layer reads from a neighbour frame ``t`` (split16 [1, H, W, cin]) -- the hi piece and the lo
    piece of chunk 0, 16 bytes each, first or ``second`` half -- alone inside a holding tensor of cin + 16 channels: the frame's chunk 0 is the
    holding tensor's chunk 1, and the other half of that chunk, every other chunk and the guards are NaN.  Returns (handle, pstride, coff)."""
    H, W = t.shape[-3:-1]
    ps, off = cin + 16, 16 + (4 if second else 0)
    g = arena._guard(H * W * ps, 1, 4)
    h = arena.Arena((H * W, 2, 4), (ps, 8, 1), g + off, g + H * W * ps + g, 0xFF, t.device)
    flat = t.reshape(-1)
    h.write(torch.as_strided(flat, (H * W, 2, 4), (cin, 8, 1), flat.storage_offset() + (4 if second else 0)))
    h.coff = off
    return h, ps, 16 + (8 if second else 0)


def _rehomed(c, a, y_shape, fill, widen_extra=0, **layout):
    x = _storage(c.x)
    hp, hn, e = c.kw.get("halo_prev"), c.kw.get("halo_next"), c.kw.get("extra")
    if layout.get("halo_layout") == "half":
        b, h = arena.rehome(a, x, y_shape, extra=e, y_fill=fill)
        for nm, halo, second in (("halo_prev", hp, True), ("halo_next", hn, False)):
            h[nm], ps, co = _half_chunk_halo(halo.t, a.Cin, second)
            setattr(b, nm, h[nm].hold_ptr)
            setattr(b, nm + "_pstride", ps)
            setattr(b, nm + "_coff", co)
        return b, h
    if layout.get("halo_layout") in ("wide", "compact"):
        layout["halo_n"] = c.sp.fold
    if widen_extra:
        layout["extra_pstride"] = a.extra_pstride + widen_extra
    return arena.rehome(a, x, y_shape, extra=e, halo_prev=None if hp is None else tuple(hp), halo_next=None if hn is None else tuple(hn),
                        y_fill=fill, **layout)


@pytest.mark.parametrize("family,lay", CASES, ids=["%s-%s" % fl for fl in CASES])
def test_rehomed_layer(family, lay):
    build, bargs, expect, _ = FAMILIES[family]
    c = build(*bargs)
    lib = c.ex.lib
    a, y = _args(c)
    rc, name_t = _variant(lib, a)
    assert rc == 0 and _declared(expect, name_t), (rc, name_t, lib.bsvd_last_error())
    _go(lib, a)
    y_tight = _storage(y).clone()
    refuses = lay == "D" and family.split()[0] != "f32"
    runs, inputs, names = [], [], set()
    for fill in (0x00, 0xFF):
        b, h = _rehomed(c, a, y_tight.shape, fill, **LAYOUTS[lay])
        rc, name = _variant(lib, b)
        if refuses:
            # the split mode and the Winograd form have no gather for a frame stride that is not a multiple of 4 elements: refused with the
            # reason, before anything is launched or written
            assert rc in (-17, -19, -20) and b"aligned" in lib.bsvd_last_error(), (rc, lib.bsvd_last_error())
            assert lib.bsvd_conv3x3(ctypes.byref(b), _stream()) == rc and b"aligned" in lib.bsvd_last_error()
            torch.cuda.synchronize()
            assert bool((h["y"].buf == fill).all()) and all(i.slack_intact() for k, i in h.items() if k != "y")
            continue
        want = "[generic]" if lay == "D" and name_t.startswith("conv3x3_kernel") else expect
        assert rc == 0 and _declared(want, name), (rc, name, lib.bsvd_last_error())
        _go(lib, b)
        names.add(name)
        runs.append(h.pop("y"))
        inputs += list(h.values())
    if refuses:
        return
    v = arena.verdict(runs, inputs, y_tight if names == {name_t} else None, c.ref, c.tol, c.decode)
    vals = [c.decode(r.logical()) if c.decode else r.logical() for r in runs]
    print("%s / %s: %s -> %s, max-abs vs the oracle %.3e (bound %.1e)" % (family, lay, name_t, sorted(names),
                                                                         float((vals[0].double().cpu() - c.ref.double()).abs().max()), c.tol))
    assert all(v.values()), (v, name_t, names, [r.slack_damage() for r in runs], [i.slack_damage() for i in inputs])
    if lay != "D":
        assert "equals_tight" in v, (name_t, names)        # same instantiation, so the bit comparison above did take place


def test_fold8_half_chunk_halo_forms_of_the_split_mode():
    """A half chunk of fp16 pairs is the compact [hi x8 | lo x8] slice or sits inside a split16 frame, where coff names the chunk and coff % 16
    is ignored (include/bsvd_hip.h): the same bits for every coff inside the chunk; a pstride that is neither form, or a chunk outside the
    pixel, is refused with the reason and launches nothing (the forms it takes are the cases 'f16x3 fold8' above)."""
    build, bargs, _, _ = FAMILIES["f16x3 fold8, frames"]
    c = build(*bargs)
    lib = c.ex.lib
    a, y = _args(c)
    _go(lib, a)
    y_tight = y.clone()
    for field, val in (("halo_prev_coff", 0), ("halo_prev_coff", 12), ("halo_next_coff", 8)):
        b = arena.copy_args(a)
        setattr(b, field, val)
        y.fill_(7.0)
        _go(lib, b)
        assert arena.same_bits(y, y_tight), (field, val)
    for field, val in (("halo_prev_pstride", 24), ("halo_next_pstride", 72), ("halo_prev_coff", 64), ("halo_next_coff", 72), ("halo_prev_coff", -8)):
        b = arena.copy_args(a)
        setattr(b, field, val)
        y.fill_(7.0)
        assert lib.bsvd_conv3x3(ctypes.byref(b), _stream()) == -17 and b"fold 8" in lib.bsvd_last_error(), (field, val, lib.bsvd_last_error())
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------ transformed-domain hand-over
# For y_v producers, bsvd_to_v and the x_v reader "every element written" is not the contract: the layout has pad groups, an edge record and
# edge lines with their own rules.  Asserted instead: nothing outside the frames' bsvd_v_frame_elems is written, and a reader fed the strided
# tensor gives the bits it gives on the tight one.

def _v_reader(T, H, W):
    from bsvd_amd.schedule import Halo
    sp, st = _v_layer(128, 128, True, "relu6", 0)
    ex = _wino_exec(_Net(sp), st, "wino6")
    ex.force_x_f32, ex.force_y_v = False, 0
    rs = np.random.RandomState(H + W)
    x, hp, hn = _randn(rs, T, H, W, 128), _randn(rs, 1, H, W, sp.fold), _randn(rs, 1, H, W, sp.fold)
    ref = OracleExecutor(st, double=True).conv(sp, x, Halo(hp[0], sp.fold, 0), Halo(hn[0], sp.fold, 0))
    return sp, ex, x, hp, hn, ref


def _v_holding(h, cin, coff, m=6):
    """the transformed slice ``h`` ([1, H, W, n] fp32) inside a transformed holding tensor of cin + 16 channels whose other chunks are NaN,
    inside an arena; returns (handle, pstride, coff)"""
    from bsvd_amd.engine import VT
    v = _to_v(h.to(_dev()), m)
    hold = VT.empty(1, v.H, v.W, cin + 16, m, _dev())
    hold.t.view(torch.uint8).fill_(0xFF)
    hold.blocks()[..., coff // 16:(coff + v.C) // 16, :].copy_(v.blocks())
    _, _, handle = arena.place(hold.t, 0)
    return handle, cin + 16, coff


def test_v_reader_on_a_strided_transformed_tensor_and_wide_transformed_halos():
    T, H, W = 3, 19, 50
    sp, ex, x, hp, hn, ref = _v_reader(T, H, W)
    from bsvd_amd.schedule import Halo
    lib = ex.lib
    xv = _to_v(x.to(_dev()), 6)
    a, y = ex.build_args(sp, xv, Halo(_to_v(hp.to(_dev()), 6)[0], sp.fold, 0), Halo(_to_v(hn.to(_dev()), 6)[0], sp.fold, 0))
    a.wino_m = 46
    rc, name_t = _variant(lib, a)
    assert rc == 0 and "winox_kernel<F(6,3)" in name_t and "[V in]" in name_t, (rc, name_t, lib.bsvd_last_error())
    _go(lib, a)
    y_tight = y.clone()
    runs, inputs = [], []
    for fill in (0x00, 0xFF):
        b, h = arena.rehome(a, xv.t, y_tight.shape, y_fill=fill)
        assert b.x_frame_stride == xv.frame_stride + 20
        for nm, t, coff in (("halo_prev", hp, 16 + sp.fold), ("halo_next", hn, 16)):
            h[nm], ps, co = _v_holding(t, 128, coff)
            setattr(b, nm, h[nm].ptr)
            setattr(b, nm + "_pstride", ps)
            setattr(b, nm + "_coff", co)
        assert _variant(lib, b) == (0, name_t), lib.bsvd_last_error()
        _go(lib, b)
        runs.append(h.pop("y"))
        inputs += list(h.values())
    v = arena.verdict(runs, inputs, y_tight, ref, WINO_TIGHT, from_split)
    assert all(v.values()) and "equals_tight" in v, (v, [r.slack_damage() for r in runs])


@pytest.mark.parametrize("x_v", [False, True])
def test_v_producer_into_a_strided_tensor_keeps_to_its_frames_and_feeds_the_same_reader_bits(x_v):
    T, H, W = 3, 19, 50
    sp, st = _v_layer(128, 128, False, "relu6", 0)
    ex = _wino_exec(_Net(sp), st, "wino6")
    lib = ex.lib
    rs = np.random.RandomState(31)
    xd = _randn(rs, T, H, W, 128).to(_dev())
    xin = _to_v(xd, 6) if x_v else xd
    ex.force_x_f32, ex.force_y_f32, ex.force_y_v = not x_v, False, 6
    a, yv = ex.build_args(sp, xin)
    a.wino_m = 46
    rc, name_t = _variant(lib, a)
    assert rc == 0 and "[V out]" in name_t and ("[V in]" in name_t) == x_v, (rc, name_t, lib.bsvd_last_error())
    _go(lib, a)
    elems = lib.bsvd_v_frame_elems(H, W, 128, 6)
    assert yv.t.shape == (T, elems)

    def read(ptr, fs):          # the reader: the same layer on a transformed input, NHWC pairs out
        ex.force_x_f32, ex.force_y_v = False, 0
        ra, ry = ex.build_args(sp, yv)
        ra.wino_m, ra.x, ra.x_frame_stride = 46, ptr, fs
        assert "[V in]" in _variant(lib, ra)[1]
        _go(lib, ra)
        return ry

    r_tight = read(yv.data_ptr(), yv.frame_stride)
    for fill in (0x00, 0xFF):
        b, h = arena.rehome(a, xin.t if x_v else xin, (T, elems), y_fill=fill)
        assert b.y_frame_stride == elems + 20 and _variant(lib, b) == (0, name_t)
        _go(lib, b)
        assert h["y"].slack_intact() and h["x"].slack_intact(), (fill, h["y"].slack_damage(), h["x"].slack_damage())
        r = read(h["y"].ptr, h["y"].frame_stride)
        assert arena.same_bits(r, r_tight), fill          # whatever the producer leaves unwritten inside a frame, no reader consumes
        assert h["y"].slack_intact()                      # ... and the reader is const on it
    want = OracleExecutor(st, double=True)
    final = want.conv(sp, want.conv(sp, xd.cpu()))
    err = float((from_split(r_tight.cpu()).double() - final.double()).abs().max())
    print("producer -> reader through the transformed domain: max-abs vs the oracle's two convs %.3e" % err)
    assert err < WINO_TIGHT * max(1.0, float(final.abs().max()))          # the bound's form in test_gpu_v_handover.py


@functools.lru_cache(maxsize=None)
def _to_v_operands(x_f32):
    """the layer whose F(m,3) readers consume bsvd_to_v's output, its logical input (the values fp16 pairs carry where x_f32 == 0) and ONE
    oracle reference for both forms"""
    T, H, W = 3, 19, 50
    sp, st = _v_layer(128, 128, False, "relu6", 0)
    x = _randn(np.random.RandomState(40 + x_f32), T, H, W, 128)
    x = x if x_f32 else _quant(x)
    return sp, st, x, OracleExecutor(st, double=True).conv(sp, x)


@pytest.mark.parametrize("m", [2, 6])
@pytest.mark.parametrize("x_f32", [0, 1])
def test_to_v_with_strided_source_and_destination(x_f32, m):
    """bsvd_to_v from a strided NHWC tensor (fp16 pairs or plain fp32) into a strided transformed tensor: nothing outside the frames is written, the
    F(m,3) reader fed the strided result is within the Winograd bound of the oracle on the logical operands and bit-equal to the reader fed the
    tight result (and so is the tensor itself: bsvd_to_v writes every element of a frame, pad groups and the edge record as zeros)."""
    from bsvd_amd import _lib
    from bsvd_amd.engine import VT
    lib = _lib.load()
    sp, st, x, ref = _to_v_operands(x_f32)
    T, H, W, C = x.shape
    ex = _wino_exec(_Net(sp), st, "wino%d" % m)
    ex.force_x_f32, ex.force_y_f32, ex.force_y_v = False, False, 0
    xd = (x if x_f32 else to_split(x)).to(_dev())
    tight = _to_v(xd, m, bool(x_f32))
    elems = VT.frame_elems(H, W, C, m)

    def read(ptr, fs):
        a, y = ex.build_args(sp, tight)
        a.wino_m, a.x, a.x_frame_stride = 40 + m, ptr, fs
        rc, name = _variant(lib, a)
        assert rc == 0 and "winox_kernel<F(%d,3)" % m in name and "[V in]" in name, (rc, name, lib.bsvd_last_error())
        _go(lib, a)
        return y

    r_tight = read(tight.data_ptr(), tight.frame_stride)
    xp, x_fs, hx = arena.place(xd, 20)
    for fill in (0x00, 0xFF):
        hv = arena.reserve((T, elems), 20, fill=fill, device=_dev())
        rc = lib.bsvd_to_v(xp, x_fs, x_f32, hv.ptr, hv.frame_stride, T, H, W, C, m, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.bsvd_last_error()
        assert hv.slack_intact(), (fill, hv.slack_damage())
        r = from_split(read(hv.ptr, hv.frame_stride).cpu())
        err = float((r.double() - ref.double()).abs().max())
        print("bsvd_to_v x_f32 %d -> F(%d,3) reader: max-abs vs the oracle %.3e (bound %.1e)" % (x_f32, m, err, WINO_TIGHT))
        assert not bool(torch.isnan(r).any()) and err < WINO_TIGHT
        assert arena.same_bits(r, from_split(r_tight.cpu()))
        assert arena.same_bits(hv.logical(), tight.t)
        assert hv.slack_intact()
    assert hx.slack_intact()


# ------------------------------------------------------------------------------------------------ layout helpers

@pytest.mark.parametrize("C", [3, 5])
def test_nchw_nhwc_helpers_in_arenas(C):
    from bsvd_amd import _lib
    lib = _lib.load()
    T, H, W, CP = 3, 14, 22, 16
    x = torch.randn(T, C, H, W, generator=torch.Generator().manual_seed(C)) * 2
    xp, _, hx = arena.place(x.to(_dev()), 0)
    outs = []
    for fill in (0x00, 0xFF):
        hd = arena.reserve((T, H, W, CP), 0, fill=fill, device=_dev())
        assert lib.bsvd_nchw_to_nhwc(xp, hd.ptr, T, C, H, W, CP, _lib.BSVD_F32, _stream()) == 0, lib.bsvd_last_error()
        torch.cuda.synchronize()
        assert hd.slack_intact() and hx.slack_intact(), hd.slack_damage()
        outs.append(hd.logical().cpu())
        # the split mode enters through the planar edge layers: the helper refuses its dtype and writes nothing
        hr = arena.reserve((T, H, W, CP), 0, fill=fill, device=_dev())
        assert lib.bsvd_nchw_to_nhwc(xp, hr.ptr, T, C, H, W, CP, _lib.BSVD_F16X3, _stream()) == -2
        torch.cuda.synchronize()
        assert bool((hr.buf == fill).all())
    want = torch.zeros(T, H, W, CP)
    want[..., :C] = x.permute(0, 2, 3, 1)
    assert arena.same_bits(outs[0], want) and arena.same_bits(outs[1], want)          # padded channels: +0 whatever dst held
    # ... and back, out of an NHWC tensor whose padded channels are NaN: they reach no result
    src = torch.full((T, H, W, CP), float("nan"))
    src[..., :C] = x.permute(0, 2, 3, 1)
    sp_, _, hs = arena.place(src.to(_dev()), 0)
    for fill in (0x00, 0xFF):
        for clamp in (0, 1):
            hd = arena.reserve((T, C, H, W), 0, fill=fill, device=_dev())
            assert lib.bsvd_nhwc_to_nchw(sp_, hd.ptr, T, C, H, W, CP, _lib.BSVD_F32, clamp, 0.0, 1.0, _stream()) == 0, lib.bsvd_last_error()
            torch.cuda.synchronize()
            assert hd.slack_intact() and hs.slack_intact(), hd.slack_damage()
            assert arena.same_bits(hd.logical().cpu(), x.clamp(0.0, 1.0) if clamp else x)
        hr = arena.reserve((T, C, H, W), 0, fill=fill, device=_dev())
        assert lib.bsvd_nhwc_to_nchw(sp_, hr.ptr, T, C, H, W, CP, _lib.BSVD_F16X3, 0, 0.0, 1.0, _stream()) == -2
        torch.cuda.synchronize()
        assert bool((hr.buf == fill).all())


@pytest.mark.parametrize("dtype,C,c0,n", [("f32", 48, 16, 16), ("f32", 48, 5, 3), ("f16x3", 48, 8, 8)])
def test_halo_pack_unpack_in_arenas(dtype, C, c0, n):
    from bsvd_amd import _lib
    lib = _lib.load()
    dt = _lib.BSVD_F32 if dtype == "f32" else _lib.BSVD_F16X3
    H, W = 10, 19                                   # 190 pixels: a multiple of no block size
    frame = torch.randn(H, W, C, generator=torch.Generator().manual_seed(n))
    if dtype == "f16x3":
        cont = to_split(frame)
        h16 = cont.view(torch.float16).reshape(H, W, C // 16, 2, 16)          # [.., chunk, hi | lo, 16]
        want = h16[:, :, c0 // 16, :, c0 % 16:c0 % 16 + 8].reshape(H, W, 16).contiguous().view(torch.float32)      # [hi x8 | lo x8]
        frame = cont
    else:
        want = frame[..., c0:c0 + n].contiguous()
    fp, _, hf = arena.place(frame[None].to(_dev()), 0)
    for fill in (0x00, 0xFF):
        hd = arena.reserve((1, H, W, n), 0, fill=fill, device=_dev())
        assert lib.bsvd_halo_pack(fp, hd.ptr, H * W, C, c0, n, dt, _stream()) == 0, lib.bsvd_last_error()
        torch.cuda.synchronize()
        assert hd.slack_intact() and hf.slack_intact(), hd.slack_damage()
        assert arena.same_bits(hd.logical()[0].cpu(), want)
        # unpack: the slice's channels of a frame are the logical elements, every other channel of the frame is slack
        if dtype == "f32":
            hu = arena.reserve_pixels((H, W, n), C, c0, fill=fill, device=_dev())
            base = hu.hold_ptr
        else:                                       # the two 16-byte pieces of the half chunk: [pixel][hi, lo][4 floats]
            off = (c0 // 16) * 16 + (c0 // 8 % 2) * 4
            g = arena._guard(H * W * C, 1, 4)
            hu = arena.Arena((H * W, 2, 4), (C, 8, 1), g + off, g + H * W * C + g, fill, _dev())
            base = hu.ptr - off * 4
        assert lib.bsvd_halo_unpack(hd.ptr, base, H * W, C, c0, n, dt, _stream()) == 0, lib.bsvd_last_error()
        torch.cuda.synchronize()
        assert hu.slack_intact() and hd.slack_intact(), hu.slack_damage()          # untouched channels and the guards
        assert arena.same_bits(hu.logical().reshape(-1).cpu(), want.reshape(-1))


# ------------------------------------------------------------------------------------------------ weight packs

def _pack_twice(call, w_bytes, b_elems):
    """one pack into a zeroed and one into a 0xFF pre-filled buffer of exactly the documented size, both inside arenas: the guards stay
    intact and the two packs have the same bits (the header's "zero-filled padding" does not lean on what the destination held)"""
    got = []
    for fill in (0x00, 0xFF):
        hw = arena.reserve((1, w_bytes), 0, fill=fill, device=_dev(), dtype=torch.uint8)
        hb = arena.reserve((1, b_elems), 0, fill=fill, device=_dev())
        assert hw.ptr % 16 == 0
        rc = call(hw.ptr, hb.ptr)
        torch.cuda.synchronize()
        assert rc == 0
        assert hw.slack_intact() and hb.slack_intact(), (fill, hw.slack_damage(), hb.slack_damage())
        got.append((hw.logical().cpu(), hb.logical().cpu()))
    assert torch.equal(got[0][0], got[1][0]) and arena.same_bits(got[0][1], got[1][1])
    assert not bool(torch.isnan(got[1][1]).any())
    return got[1]


PACK_SHAPES = [(30, 64, 32, 64), (64, 3, 64, 16), (24, 40, 32, 48)]      # Cin, Cout, Cin_pad, Cout_pad: every one needs padding


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
@pytest.mark.parametrize("cin,cout,cin_pad,cout_pad", PACK_SHAPES + [(24, 40, 32, 64)])
def test_pack_weights_in_arenas(cin, cout, cin_pad, cout_pad, dtype, with_bias):
    from bsvd_amd import _lib
    from test_gpu_pack_layout import expect_pack, weights
    lib = _lib.load()
    ps = 1 if cout_pad == 64 and cout == 40 else 0          # 40 channels as 4 x 10 PixelShuffle sub-pixel groups padded to 4 x 16
    w, bias = weights(3, cin, cout)
    wd, bd = torch.from_numpy(w).to(_dev()), torch.from_numpy(bias).to(_dev())
    dt = _lib.BSVD_F32 if dtype == "f32" else _lib.BSVD_F16X3
    nbytes = 4 * lib.bsvd_packed_weight_elems(cin_pad, cout_pad)
    gw, gb = _pack_twice(lambda wp, bp: lib.bsvd_pack_weights(wd.data_ptr(), bd.data_ptr() if with_bias else None, cin, cout, cin_pad, cout_pad,
                                                              ps, dt, wp, bp, _stream()), nbytes, cout_pad)
    ew, eb = expect_pack(w, bias if with_bias else None, cin_pad, cout_pad, ps, dt)
    assert np.array_equal(gw.numpy().reshape(-1), np.ascontiguousarray(ew).view(np.uint8).reshape(-1))
    assert np.array_equal(gb.numpy().reshape(-1).view(np.uint8), eb.view(np.uint8))


@pytest.mark.parametrize("m", [2, 6])
@pytest.mark.parametrize("cin,cout,cin_pad,cout_pad,ps", [(30, 64, 32, 64, 0), (24, 40, 32, 64, 0), (24, 40, 32, 64, 1), (64, 3, 64, 32, 0)])
def test_pack_weights_wino_in_arenas(cin, cout, cin_pad, cout_pad, ps, m):
    from bsvd_amd import _lib
    from test_gpu_pack_layout import weights
    lib = _lib.load()
    w, bias = weights(4, cin, cout)
    wd, bd = torch.from_numpy(w).to(_dev()), torch.from_numpy(bias).to(_dev())
    nbytes = 4 * lib.bsvd_packed_wino_weight_elems(cin_pad, cout_pad, m)
    gw, gb = _pack_twice(lambda wp, bp: lib.bsvd_pack_weights_wino(wd.data_ptr(), bd.data_ptr(), cin, cout, cin_pad, cout_pad, ps, m, wp, bp,
                                                                   _stream()), nbytes, cout_pad)
    # (the bytes themselves are tests/test_gpu_pack_layout.py's; here: which channels are padding -- [Cin_pad/16][m+2][3][hi, lo][2][Cout_pad][8])
    h = gw.view(torch.float16).reshape(cin_pad // 16, m + 2, 3, 2, 2, cout_pad, 8).float()
    real_n = torch.zeros(cout_pad, dtype=torch.bool)
    for n in range(cout):
        real_n[(n % 4) * (cout_pad // 4) + n // 4 if ps else n] = True
    assert not bool(h[..., ~real_n, :].any()) and not bool(torch.isnan(h).any())
    cpad = h.permute(0, 4, 6, 1, 2, 3, 5).reshape(cin_pad, -1)[cin:]            # input channel = chunk * 16 + h * 8 + j
    assert not bool(cpad.any())
    assert not bool(gb.reshape(-1)[~real_n].any()) and bool(h[..., real_n, :].any())


@pytest.mark.parametrize("with_bias", [True, False])
def test_pack_head_weights_in_arenas(with_bias):
    from bsvd_amd import _lib
    from test_gpu_pack_layout import expect_head, weights
    lib = _lib.load()
    cin, cmid, cmid_pad = 3, 30, 32
    w, bias = weights(5, cin, cmid)
    wd, bd = torch.from_numpy(w).to(_dev()), torch.from_numpy(bias).to(_dev())
    gw, gb = _pack_twice(lambda wp, bp: lib.bsvd_pack_head_weights(wd.data_ptr(), bd.data_ptr() if with_bias else None, cin, cmid, cmid_pad, wp, bp,
                                                                   _stream()), lib.bsvd_packed_head_weight_bytes(cmid_pad), cmid_pad)
    ew, eb = expect_head(w, bias if with_bias else None, cmid_pad)
    assert np.array_equal(gw.numpy().reshape(-1), np.ascontiguousarray(ew).view(np.uint8).reshape(-1))
    assert np.array_equal(gb.numpy().reshape(-1).view(np.uint8), eb.view(np.uint8))
