"""Pass-isolating probes of the split-fp16 mode (BSVD_F16X3): every MFMA pass and every `lo` half at full strength.

The layer tests draw unit-scale canonical pairs, where the `lo` halves and two of the three passes (lo.hi, hi.lo) contribute 2^-11 of
the result: a `lo`-path fault confined to one chunk of K stays under their flat tolerance.  The direct-form kernels are LINEAR in the
two halves of a container and the tests build the containers, so here the halves are chosen freely:

  hi_only      (hi = v, lo = 0)            must give conv(v, w_hi + w_lo)
  lo_only      (hi = 0, lo = v)            must give conv(v, w_hi) and nothing else (there is no lo.lo pass): a lo-path fault shows at O(1)
  independent  (hi = a, lo = b), |b| ~ |a| against the three-pass model of both halves
  lo_plane     weights c + r, |r| < ulp(c) / 2: w_hi is constant, all the information is in w_lo (the hi.lo_w pass, the packer's lo plane)

through temporal halos in the three forms the schedules use (none, compact [H][W][fold], full neighbour frame; fold 16 / 32 and the fold-8
half chunk [hi x8 | lo x8]), the PS_ADD skip tensor, the split RESID base and bsvd_halo_pack / bsvd_halo_unpack.  The Winograd kernels
decode hi + lo before they transform, so their property is: containers with the same hi + lo give the same result, a container whose
information is all in `lo` matches the model, and the weight-side probe goes through bsvd_pack_weights_wino.

Reference: tests/split_model.py (float64 three-pass model; tests/test_split_model_cpu.py pins it and proves that the bound below catches a
dropped pass, a zeroed / swapped lo chunk and flushed subnormals).  Tolerance, elementwise:

    |gpu - model| <= m x (max error of a plain float32 accumulation chain on the same operands) + 2^-22 |y| + 2^-24

with ONE m for the direct-form kernels (split_model.M_DIRECT = 2) and one per Winograd form against the float32 Winograd algorithm
(split_model.M_WINO = {2: 1, 6: 2}): the smallest powers of two the product kernels pass with on the MI355X.  The measured ratios per
kernel family are in profiles/f16x3_value_probes.txt (direct-form families 0.41 - 0.78, the planar exit with a split base 1.007; F(2,3)
0.69; F(6,3) 1.07).  Every case prints the margin it needs before it asserts.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import split_model as S
from seeded import seeded_state
from test_gpu_f16x3 import _Net, _exec

pytestmark = pytest.mark.gpu
M, M_WINO = S.M_DIRECT, S.M_WINO


def _dev():
    return torch.device("cuda", 0)


def _state(sp, rs, kind="kaiming", wino_m=None):
    st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 7)
    shape = (sp.cout, sp.cin, 3, 3)
    if kind == "lo_plane":
        st[sp.key + ".weight"] = S.lo_plane_weights(shape, rs)
    else:
        st[sp.key + ".weight"] = (rs.standard_normal(shape) * (2.0 / (9 * sp.cin)) ** 0.5).astype(np.float32)
    if wino_m:        # the Winograd model is defined up to rounding ties of U = G g: none in the test's weights (split_model.detie_wino_weights)
        st[sp.key + ".weight"] = S.detie_wino_weights(st[sp.key + ".weight"], wino_m)
    st[sp.key + ".bias"] = (rs.standard_normal(sp.cout) * 0.1).astype(np.float32)
    return st


def _halves(kind, shape, rs):
    """fp16-valued (hi, lo) of one activation tensor for probe `kind`"""
    if kind in ("canonical", "lo_plane"):
        return S.pairs(rs.standard_normal(shape).astype(np.float32))
    v = S.fp16(rs.standard_normal(shape))
    if kind == "hi_only":
        return v, np.zeros_like(v)
    if kind == "lo_only":
        return np.zeros_like(v), v
    assert kind == "independent"
    return v, S.fp16(rs.standard_normal(shape))


PROBES = ["hi_only", "lo_only", "independent", "lo_plane"]

FAMILIES = OrderedDict([
    # name: (cin, cout, stride, tsm, act, epi, T, H, W, fat_min_wgs, the kernel instantiation that must run)
    ("tile64", (64, 64, 1, False, "relu6", 0, 2, 33, 50, 0, "conv3x3_kernel<4,1,2,2,1>[f16x3]")),          # ragged in x and y, frames 2
    ("tile64 edge column", (64, 64, 1, False, "relu", 0, 1, 18, 33, 0, "conv3x3_kernel<4,1,2,2,1>[f16x3]")),   # one live column / two live rows in the last tiles
    ("tile64 resid", (64, 64, 1, False, "none", 2, 2, 12, 20, 0, "conv3x3_kernel<4,1,2,2,1>[f16x3]")),
    ("fold8", (64, 64, 1, True, "relu6", 0, 3, 10, 19, 0, "conv3x3_kernel<2,2,4,1,1>[f16x3][fold8]")),
    ("fold8 one frame", (64, 64, 1, True, "relu", 0, 1, 21, 36, 0, "conv3x3_kernel<2,2,4,1,1>[f16x3][fold8]")),
    ("tile128 fold16", (128, 128, 1, True, "relu6", 0, 3, 10, 19, 0, "conv3x3_kernel<2,2,2,2,1>[f16x3]")),
    ("tile128 fold32", (256, 256, 1, True, "relu", 0, 2, 9, 17, 0, "conv3x3_kernel<2,2,2,2,1>[f16x3]")),
    ("fat fold16", (128, 128, 1, True, "relu6", 0, 2, 24, 33, 1, "conv3x3_kernel<4,2,2,2,1>[f16x3]")),     # last-row band: the lower wave pair below the image
    ("fat ps_add", (128, 256, 1, False, "none", 1, 1, 17, 20, 1, "conv3x3_kernel<4,2,2,2,1>[f16x3]")),
    ("stride2 64-128", (64, 128, 2, False, "relu6", 0, 2, 20, 36, 0, "conv3x3_kernel<4,1,1,4,2>[f16x3]")),
    ("stride2 128-256", (128, 256, 2, False, "relu6", 0, 1, 27, 43, 0, "conv3x3_kernel<4,1,1,4,2>[f16x3]")),
    ("ps_add 256-512", (256, 512, 1, False, "none", 1, 2, 9, 13, 0, "conv3x3_kernel<2,2,2,2,1>[f16x3]")),
    ("ps_add 128-256", (128, 256, 1, False, "none", 1, 1, 12, 20, 0, "conv3x3_kernel<2,2,2,2,1>[f16x3]")),
])


def _halo_forms(sp, kind, T, H, W, rs):
    """[(tag, prev, next)]: each a pair of Halos (hi values, lo values) or None -- none, compact slices, full neighbour frames"""
    from bsvd_amd.schedule import Halo
    forms = [("no halo", None, None)]
    if sp.tsm:
        f, cin = sp.fold, sp.cin
        ph, pl = _halves(kind, (H, W, f), rs)
        nh, nl = _halves(kind, (H, W, f), rs)
        forms.append(("compact", (Halo(ph, f, 0), Halo(pl, f, 0)), (Halo(nh, f, 0), Halo(nl, f, 0))))
        fh, fl = _halves(kind, (1, H, W, cin), rs)
        forms.append(("full frame", (Halo(fh, cin, f), Halo(fl, cin, f)), (Halo(fh, cin, 0), Halo(fl, cin, 0))))
    return forms


def _dev_halo(h):
    from bsvd_amd.schedule import Halo
    return None if h is None else Halo(S.container(h[0].t, h[1].t).to(_dev()), h[0].pstride, h[0].coff)


def _report(tag, need, m, err, y):
    print("NEED | %s | %.3f | margin %d | chain err %.2e | max|y| %.2f" % (tag, need, m, err, y))


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_direct_form_probes(family, probe):
    from bsvd_amd.netspec import ConvSpec
    cin, cout, stride, tsm, act, epi, T, H, W, fat, variant = FAMILIES[family]
    rs = np.random.RandomState(len(family) * 131 + PROBES.index(probe) + cin + H)
    sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
    st = _state(sp, rs, probe)
    w, b = st["l.weight"], st["l.bias"]
    gex = _exec(_Net(sp), st)
    gex.fat_min_wgs = fat
    gex.record_variants = True
    xh, xl = _halves(probe, (T, H, W, cin), rs)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw, extra_dev = {}, None
    if epi == 1:          # the skip tensor is a container too: its halves follow the probe
        eh, el = _halves(probe, (T, 2 * Ho, 2 * Wo, cout // 4), rs)
        kw = dict(extra=eh + el, extra_pstride=cout // 4, extra_cstride=1)
        extra_dev = S.container(eh, el).to(_dev())
    elif epi == 2:        # the residual base of DenBlock 1: the planar fp32 network input
        base = rs.standard_normal((T, 4, Ho, Wo)).astype(np.float32)
        kw = dict(extra=base, extra_pstride=1, extra_cstride=Ho * Wo)
        extra_dev = torch.from_numpy(base).to(_dev())
    for tag, hp, hn in _halo_forms(sp, probe, T, H, W, rs):
        model = S.direct_three_pass(sp, xh, xl, w, b, hp, hn, **kw)
        err = S.chain_err(sp, xh + xl, w, b, halo_prev=S._sum_halo(hp), halo_next=S._sum_halo(hn), **kw)
        got = gex.conv(sp, S.container(xh, xl).to(_dev()), _dev_halo(hp), _dev_halo(hn), extra_dev, kw.get("extra_pstride", 0),
                       kw.get("extra_cstride", 1))
        assert gex.last_variant.startswith(variant) and "[generic]" not in gex.last_variant, gex.last_variant
        gh, gl = S.halves(got.cpu())
        need = S.needed(gh + gl, model, err)
        _report("%s | %s | %s" % (family, probe, tag), need, M, err, float(model.abs().max()))
        assert float(model.abs().max()) > 0.1            # the probe is not vacuous
        assert need <= M, (family, probe, tag, need)
        if probe == "lo_only" and epi == 0:
            # ... "and nothing else": against the plain float64 conv of v with w_hi, not only the model's own path
            ref = S.conv_f64(sp, xl, S.pairs(w)[0], b, S._h(hp, 1), S._h(hn, 1))
            assert S.needed(gh + gl, ref, err) <= M
        if probe == "hi_only" and epi == 0:
            ref = S.conv_f64(sp, xh, sum(S.pairs(w)), b, S._h(hp, 0), S._h(hn, 0))
            assert S.needed(gh + gl, ref, err) <= M


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("base_split", [False, True])
def test_planar_exit_probes(probe, base_split):
    """the network's exit: 64 -> 3, RESID, planar fp32 output; its base is the planar fp32 input (DenBlock 1) or an engine tensor whose two
    halves the epilogue decodes (BsvdConvArgs.extra_split)"""
    from bsvd_amd.netspec import ConvSpec
    T, H, W = 2, 21, 37
    rs = np.random.RandomState(17 + PROBES.index(probe) + 2 * base_split)
    sp = ConvSpec("l", "l", 64, 3, 1, False, "none", 2)
    st = _state(sp, rs, probe)
    w, b = st["l.weight"], st["l.bias"]
    gex = _exec(_Net(sp), st)
    gex.record_variants = True
    xh, xl = _halves(probe, (T, H, W, 64), rs)
    if base_split:
        eh, el = _halves(probe, (T, H, W, 64), rs)
        kw = dict(extra=eh + el, extra_pstride=64, extra_cstride=1)
        extra_dev = S.container(eh, el).to(_dev())
    else:
        base = rs.standard_normal((T, 4, H, W)).astype(np.float32)
        kw = dict(extra=base, extra_pstride=1, extra_cstride=H * W)
        extra_dev = torch.from_numpy(base).to(_dev())
    for clamp in (None, (0.0, 1.0)):
        model = S.direct_three_pass(sp, xh, xl, w, b, y_planar=(3, clamp), **kw)
        err = S.chain_err(sp, xh + xl, w, b, y_planar=(3, clamp), **kw)
        got = gex.conv(sp, S.container(xh, xl).to(_dev()), extra=extra_dev, extra_pstride=kw["extra_pstride"], extra_cstride=kw["extra_cstride"],
                       y_planar=(3, clamp))
        assert gex.last_variant.startswith("conv3x3_kernel<2,1,4,1,1>[f16x3][planar out]"), gex.last_variant
        assert got.shape == (T, 3, H, W)
        need = S.needed(got.cpu(), model, err)
        _report("planar exit %s base | %s | clamp %s" % ("split" if base_split else "planar", probe, clamp), need, M, err, float(model.abs().max()))
        assert need <= M, (probe, base_split, clamp, need)


def _pair_chain(a, b, x, wa, ba, wb, bb):
    """the two convs as float32 chains (the tensor between them stays float32) against float64: the yardstick of the fused launches"""
    y1c, y1d = S.fp32_chain(a, x, wa, ba)
    y2c, _ = S.fp32_chain(b, y1c.float().double(), wb, bb)
    return float((y2c - S.conv_f64(b, y1d, wb, bb)).abs().max())


@pytest.mark.parametrize("probe", ["hi_only", "lo_only", "independent"])
@pytest.mark.parametrize("ca,cm,cb,act,T,H,W", [(64, 64, 64, "relu6", 2, 10, 19), (64, 32, 64, "relu", 1, 33, 50)])
def test_fused_pair_probes(ca, cm, cb, act, T, H, W, probe):
    """BsvdConvArgs.pre_w_packed: probes on x; the tensor between the two convs is re-split inside the kernel"""
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import ConvSpec
    from test_gpu_pair import _PairNet
    rs = np.random.RandomState(ca + cm + H + PROBES.index(probe))
    a = ConvSpec("out0", "a", ca, cm, 1, False, act, 0)
    b = ConvSpec("out3", "b", cm, cb, 1, False, act, 0)
    st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 5)
    for sp in (a, b):
        st.update({k: v for k, v in _state(sp, rs).items() if k.startswith(sp.key + ".")})
    net = _PairNet(a, b)
    fused = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3", "direct", fuse_pairs=True))
    assert fused.fuse_pair(net.temp1, "out0", "out3")
    xh, xl = _halves(probe, (T, H, W, ca), rs)
    mid = S.direct_three_pass(a, xh, xl, st["a.weight"], st["a.bias"])
    model = S.direct_three_pass(b, *S.pairs(mid), st["b.weight"], st["b.bias"])
    err = _pair_chain(a, b, xh + xl, st["a.weight"], st["a.bias"], st["b.weight"], st["b.bias"])
    fused.record_variants = True
    got = fused.conv_pair_fused(a, b, S.container(xh, xl).to(_dev()))
    assert "[fused pair]" in fused.last_variant, fused.last_variant
    need = S.needed(sum(S.halves(got.cpu())), model, err)
    _report("fused pair %d-%d-%d | %s | -" % (ca, cm, cb, probe), need, M, err, float(model.abs().max()))
    assert float(model.abs().max()) > 0.1 and need <= M, need


@pytest.mark.parametrize("kind", ["kaiming", "lo_plane"])
@pytest.mark.parametrize("cin,cmid,cout,act,T,H,W", [(4, 64, 64, "relu6", 2, 20, 36), (3, 30, 64, "relu", 2, 17, 21)])
def test_fused_entry_probes(cin, cmid, cout, act, T, H, W, kind):
    """BsvdConvArgs.head_w_packed: the input is the caller's planar fp32 tensor (split inside the kernel), so the weight-side probe is the one
    that applies -- on both convs' packs (bsvd_pack_head_weights, bsvd_pack_weights)"""
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import ConvSpec

    class Net:
        pass

    rs = np.random.RandomState(cin + cmid + H + (kind == "lo_plane"))
    sp0 = ConvSpec("inc0", "b.inc.convblock.0", cin, cmid, 1, False, act, 0)
    sp3 = ConvSpec("inc3", "b.inc.convblock.3", cmid, cout, 1, False, act, 0)
    net = Net()
    net.layers = [sp0, sp3]
    net.temp1 = {"inc0": sp0, "inc3": sp3}
    st = {}
    for sp in (sp0, sp3):
        st.update({k: v for k, v in _state(sp, rs, kind).items() if k.startswith(sp.key + ".")})
    ex = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3"))
    assert ex.fuse_head(net.temp1)
    x = rs.standard_normal((T, cin, H, W)).astype(np.float32)
    xh, xl = S.pairs(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    w0, b0, w3, b3 = (st[sp0.key + ".weight"], st[sp0.key + ".bias"], st[sp3.key + ".weight"], st[sp3.key + ".bias"])
    mid = S.direct_three_pass(sp0, xh, xl, w0, b0)[..., :cmid]
    mh, ml = S.pairs(mid)
    pad = lambda t: np.concatenate([t, np.zeros(t.shape[:-1] + (sp3.cin_pad - cmid,))], axis=-1)
    model = S.direct_three_pass(sp3, pad(mh), pad(ml), w3, b3)
    err = _pair_chain(sp0, sp3, xh + xl, w0, b0, w3, b3)
    ex.record_variants = True
    got = ex.conv_head_fused(sp0, sp3, torch.from_numpy(x).to(_dev()))
    assert "[fused entry]" in ex.last_variant, ex.last_variant
    need = S.needed(sum(S.halves(got.cpu())), model, err)
    _report("fused entry %d-%d-%d | %s weights | -" % (cin, cmid, cout, kind), need, M, err, float(model.abs().max()))
    assert float(model.abs().max()) > 0.1 and need <= M, need


@pytest.mark.parametrize("C,fold", [(64, 8), (128, 16), (256, 32)])
def test_halo_pack_and_unpack_move_both_halves(C, fold):
    """bsvd_halo_pack / bsvd_halo_unpack on containers whose halves are unrelated: the slice is [hi | lo] of exactly those channels, bit for
    bit (fold 8: the half chunk [hi x8 | lo x8], dtype BSVD_F16X3; whole chunks travel as plain 64-byte ranges)"""
    rs = np.random.RandomState(C)
    H, W = 5, 7
    hi, lo = _halves("independent", (H, W, C), rs)
    sp_st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("l.weight", (C, C, 3, 3)), ("l.bias", (C,)),
                          ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 7)
    from bsvd_amd.netspec import ConvSpec
    gex = _exec(_Net(ConvSpec("l", "l", C, C, 1, True, "relu6", 0)), sp_st)
    frame = S.container(hi, lo).to(_dev())
    for c0 in (0, fold):
        sl = gex.halo_pack(frame, c0, fold)
        want = S.container(hi[..., c0:c0 + fold], lo[..., c0:c0 + fold])
        assert torch.equal(sl.cpu().view(torch.int32), want.view(torch.int32)), (C, fold, c0)
        h2, l2 = _halves("independent", (H, W, C), rs)
        dst = S.container(h2, l2).to(_dev())
        gex.halo_unpack(sl, dst, c0)
        h2[..., c0:c0 + fold], l2[..., c0:c0 + fold] = hi[..., c0:c0 + fold], lo[..., c0:c0 + fold]
        assert torch.equal(dst.cpu().view(torch.int32), S.container(h2, l2).view(torch.int32)), (C, fold, c0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Winograd forms

WINO_CASES = [
    # cin, cout, tsm, act, epi, T, H, W
    (128, 128, True, "relu6", 0, 3, 10, 19),        # ragged in x and y, three temporal sources
    (256, 256, True, "relu", 0, 2, 9, 17),
    (128, 128, False, "none", 0, 1, 35, 26),        # several sub-tile rows, a last-row band
    (256, 512, False, "none", 1, 2, 9, 13),         # PixelShuffle + skip add
]


def _same_sum_containers(shape, rs):
    """three pairs of halves with the SAME hi + lo: the canonical pair, a coarse hi with the rest in lo, and that one with an exactly
    representable d moved from hi to lo.  hi on the 2^-6 grid below 3, lo on the 2^-10 grid below 2^-7, d on the 2^-6 grid below 1: every half
    is an fp16 value and hi + lo is exact in fp32 (12 bits)."""
    hi = np.round(np.clip(rs.standard_normal(shape), -3, 3) * 64) / 64
    lo = rs.randint(-7, 8, shape) / 1024.0
    d = rs.randint(-63, 64, shape) / 64.0
    x = hi + lo
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x, [S.pairs(x), (hi, lo), (hi - d, lo + d)]


def _lo_only_container(shape, rs):
    """hi = the constant 1, all the information in lo (2^-12 grid below 1/2: hi + lo exact in fp32)"""
    lo = rs.randint(-2047, 2048, shape) / 4096.0
    return 1.0 + lo, [(np.ones(shape), lo)]


@pytest.mark.parametrize("probe", ["same_sum", "lo_info", "lo_plane"])
@pytest.mark.parametrize("form", ["wino2", "wino6"])
@pytest.mark.parametrize("cin,cout,tsm,act,epi,T,H,W", WINO_CASES)
def test_wino_probes(cin, cout, tsm, act, epi, T, H, W, form, probe):
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    from test_gpu_wino import _exec as _wexec
    m = int(form[4])
    rs = np.random.RandomState(cin + cout + H + m + len(probe))
    sp = ConvSpec("l", "l", cin, cout, 1, tsm, act, epi)
    st = _state(sp, rs, probe, m)
    w, b = st["l.weight"], st["l.bias"]
    gex = _wexec(_Net(sp), st, form)
    assert "l" in gex.packed.wino
    gex.force_x_f32 = gex.force_y_f32 = False
    gex.record_variants = True
    make = {"same_sum": _same_sum_containers, "lo_info": _lo_only_container,
            "lo_plane": lambda shape, r: (lambda h, l: (h + l, [(h, l)]))(*S.pairs(r.standard_normal(shape).astype(np.float32)))}[probe]
    x, conts = make((T, H, W, cin), rs)
    kw, extra_dev = {}, None
    if epi == 1:
        e, ec = make((T, 2 * H, 2 * W, cout // 4), rs)
        kw = dict(extra=e, extra_pstride=cout // 4, extra_cstride=1)
        extra_dev = S.container(*ec[-1]).to(_dev())
    forms = [("no halo", None, None, [None] * len(conts), [None] * len(conts))]
    if tsm:
        f = sp.fold
        p, pc = make((H, W, f), rs)
        n, nc = make((H, W, f), rs)
        forms.append(("compact", Halo(p, f, 0), Halo(n, f, 0), [Halo(S.container(*c).to(_dev()), f, 0) for c in pc],
                      [Halo(S.container(*c).to(_dev()), f, 0) for c in nc]))
        fr, fc = make((1, H, W, cin), rs)
        forms.append(("full frame", Halo(fr, cin, f), Halo(fr, cin, 0), [Halo(S.container(*c).to(_dev()), cin, f) for c in fc],
                      [Halo(S.container(*c).to(_dev()), cin, 0) for c in fc]))
    for tag, hp, hn, hpd, hnd in forms:
        model = S.wino_model(sp, x, w, m, b, hp, hn, **kw)
        err = S.wino_err(sp, x, w, m, b, halo_prev=hp, halo_next=hn, **kw)
        outs = []
        for i, c in enumerate(conts):
            got = gex.conv(sp, S.container(*c).to(_dev()), hpd[i], hnd[i], extra_dev, kw.get("extra_pstride", 0), kw.get("extra_cstride", 1))
            assert "_kernel<F(%d,3)" % m in gex.last_variant and "in]" not in gex.last_variant, gex.last_variant
            outs.append(got)
            need = S.needed(sum(S.halves(got.cpu())), model, err)
            _report("%s %d-%d epi %d | %s #%d | %s" % (form, cin, cout, epi, probe, i, tag), need, M_WINO[m], err, float(model.abs().max()))
            assert float(model.abs().max()) > 0.1 and need <= M_WINO[m], (form, probe, i, tag, need)
        print("    containers with the same hi + lo: %s" % ("bit-identical results" if all(torch.equal(outs[0], o) for o in outs[1:]) else "results differ"))


@pytest.mark.parametrize("reader", ["f32", "v"])
@pytest.mark.parametrize("kind", ["kaiming", "lo_plane"])
@pytest.mark.parametrize("form", ["wino2", "wino6"])
@pytest.mark.parametrize("cin,cout,tsm,act,epi,T,H,W", WINO_CASES[:2] + WINO_CASES[3:])
def test_wino_fp32_and_transformed_readers(cin, cout, tsm, act, epi, T, H, W, form, kind, reader):
    """the readers that take no pairs: plain fp32 input (x_f32) and, for F(6,3), the transformed-domain input (x_v) -- the weight-side probe and
    ordinary data against the same model.  F(2,3) has no transformed-domain reader in the product: its `v` point runs the fp32 reader with
    fp32 OUTPUT (y_f32), the other plain-fp32 hand-over."""
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    from test_gpu_v_handover import _to_v
    from test_gpu_wino import _exec as _wexec
    m = int(form[4])
    rs = np.random.RandomState(cin + cout + H + m + len(kind) + len(reader))
    sp = ConvSpec("l", "l", cin, cout, 1, tsm, act, epi)
    st = _state(sp, rs, kind, m)
    w, b = st["l.weight"], st["l.bias"]
    gex = _wexec(_Net(sp), st, form)
    gex.record_variants = True
    use_v = reader == "v" and m == 6
    y_f32 = reader == "v" and m == 2
    x = rs.standard_normal((T, H, W, cin)).astype(np.float32)
    kw, extra_dev = {}, None
    if epi == 1:
        eh, el = S.pairs(rs.standard_normal((T, 2 * H, 2 * W, cout // 4)).astype(np.float32))
        kw = dict(extra=eh + el, extra_pstride=cout // 4, extra_cstride=1)
        extra_dev = S.container(eh, el).to(_dev())
    dev = lambda t: _to_v(torch.from_numpy(t).to(_dev()), 6) if use_v else torch.from_numpy(t).to(_dev())
    forms = [("no halo", None, None, None, None)]
    if tsm:
        f = sp.fold
        p, n = rs.standard_normal((1, H, W, f)).astype(np.float32), rs.standard_normal((1, H, W, f)).astype(np.float32)
        forms.append(("compact", Halo(p[0], f, 0), Halo(n[0], f, 0), Halo(dev(p)[0], f, 0), Halo(dev(n)[0], f, 0)))
        fr = rs.standard_normal((1, H, W, cin)).astype(np.float32)
        fd = dev(fr)[0]
        forms.append(("full frame", Halo(fr[0], cin, f), Halo(fr[0], cin, 0), Halo(fd, cin, f), Halo(fd, cin, 0)))
    for tag, hp, hn, hpd, hnd in forms:
        model = S.wino_model(sp, x, w, m, b, hp, hn, **kw)
        err = S.wino_err(sp, x, w, m, b, halo_prev=hp, halo_next=hn, **kw)
        gex.force_x_f32, gex.force_y_f32, gex.force_y_v = (not use_v), y_f32, 0
        got = gex.conv(sp, dev(x), hpd, hnd, extra_dev, kw.get("extra_pstride", 0), kw.get("extra_cstride", 1))
        assert ("[V in]" if use_v else "[f32 in]") in gex.last_variant and "F(%d,3)" % m in gex.last_variant, gex.last_variant
        val = got.cpu().double() if y_f32 else sum(S.halves(got.cpu()))
        need = S.needed(val, model, err)
        _report("%s %d-%d epi %d %s | %s weights | %s" % (form, cin, cout, epi, gex.last_variant[gex.last_variant.index("]") + 1:], kind, tag),
                need, M_WINO[m], err, float(model.abs().max()))
        assert float(model.abs().max()) > 0.1 and need <= M_WINO[m], (form, kind, reader, tag, need)
