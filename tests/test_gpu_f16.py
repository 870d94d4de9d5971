"""precision='f16' (ABI BSVD_F16) on the MI355X: ONE fp16 MFMA pass, hi(w) x hi(x), on the tensors, packs, halos and epilogues of BSVD_F16X3.

Per kernel family (every direct-form split tile launch_conv3x3 selects, the fused entry, the F(2,3) Winograd kernel in every variant the
product launches):
  (a) within split_model.bound -- the three-pass mode's margins, M_DIRECT and M_WINO[2] -- of the one-pass model (tests/f16_model.py);
      tests/test_f16_cpu.py shows that the three-pass model is > 10 bounds away, so (a) tells the modes apart
  (b) decoded and compared by value, equal to the BSVD_F16X3 launch on the same tensors with x_lo = 0 and a pack made from fp16(w): the
      two passes that are left out add exact zeros there (same bits up to the sign of zero)
  (c) with every `lo` half of x, of both halos and of the fold-8 slice replaced by fp16 NaN the result is finite and equal to (b): no `lo`
      half reaches an MFMA operand.  The skip / residual operands are read as full pairs and keep real `lo` halves: stated separately.
Every case prints the margin it needs ("NEED | ...") before it asserts.

Two families are compared through a tensor that the kernel rounds to fp16 on the way -- the fused entry's middle tensor, the Winograd
form's transformed values V = BT d.  One pass has no `lo` to absorb a rounding that falls on the other side in the model (float64) than in
the kernel (fp32): one fp16 ulp of such a value is 2^-11 of it, hundreds of bounds.  Their operands are therefore drawn on dyadic grids on
which that tensor is EXACT in fp32, so model and kernel round the same number; everything behind the rounding is held to the bound.
(netspec gives a 64-channel layer fold 8 and a 128-channel one fold 16: the "both halo forms" rows of fold 16 are the 128 -> 128 ones.)

Whole networks: clip == per-frame stream == chunked stream == graph-replayed stream == 2-shard run bit for bit within the mode; max-abs
against the fp32 CPU oracle at most 2 x that of the CPU emulation of the mode (f16_model.F16EmuExecutor; the factor 2: rounding ties fall
differently under fp32 accumulation) -- computed here, never a recorded number; the PSNR proxy of tests/test_gpu_eval.py restated at 0.02 dB.
Figures measured on the MI355X: profiles/f16_one_pass.txt.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

import f16_model as F
import split_model as S
from helpers import bsvd_keys
from seeded import seeded_state
from test_gpu_f16x3 import _Net
from test_gpu_split_passes import _dev, _halo_forms, _halves, _state

pytestmark = pytest.mark.gpu
NAN16 = float("nan")


def _execs(net, st, wide="direct", fat=0):
    """(the one-pass executor, the three-pass executor on packs made from fp16(w) -- every w_lo is zero)"""
    from bsvd_amd.engine import HipExecutor, PackedNet
    t = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
    st_hi = {k: (S.fp16(v).astype(np.float32) if k.endswith(".weight") else v) for k, v in st.items()}
    e1 = HipExecutor(PackedNet(net, t(st), _dev(), "f16", wide))
    e3 = HipExecutor(PackedNet(net, t(st_hi), _dev(), "f16x3", wide))
    for e in (e1, e3):
        e.fat_min_wgs = fat
        e.record_variants = True
        e.force_x_f32 = e.force_y_f32 = False
    return e1, e3


def _cont(hi, lo=None):
    """split16 container of fp16-valued halves; lo = None: every lo half is an fp16 NaN"""
    if lo is not None:
        return S.container(hi, lo)
    hi = torch.as_tensor(S._np(hi))
    *lead, C = hi.shape
    G = 16 if C % 16 == 0 else 8
    h = hi.reshape(*lead, C // G, G).to(torch.float16)
    return torch.cat([h, torch.full_like(h, NAN16)], dim=-1).contiguous().view(torch.float32).reshape(*lead, C)


def _halo(h, lo):
    """device Halo of a (hi values, lo values) pair of Halos: lo 'real' | 'zero' | 'nan'"""
    from bsvd_amd.schedule import Halo
    if h is None:
        return None
    hi = S._np(h[0].t)
    c = _cont(hi, {"real": S._np(h[1].t), "zero": np.zeros_like(hi), "nan": None}[lo])
    return Halo(c.to(_dev()), h[0].pstride, h[0].coff)


def _values_equal(a, b):
    """two results compared half by half, by VALUE (+0 == -0)"""
    return all(np.array_equal(x, y) for x, y in zip(S.halves(a.cpu()), S.halves(b.cpu())))


def _report(tag, need, m, err, y):
    print("NEED | %s | %.3f | margin %d | chain err %.2e | max|y| %.2f" % (tag, need, m, err, y))


# name: (cin, cout, stride, tsm, act, epi, T, [(H, W)], fat_min_wgs, the instantiation that must run)
DIRECT = {
    "64-64": (64, 64, 1, False, "relu6", 0, 3, [(20, 24), (21, 37)], 0, "conv3x3_kernel<4,1,2,2,1>[f16]"),
    "128-128 fold16": (128, 128, 1, True, "relu6", 0, 3, [(20, 24), (21, 19)], 0, "conv3x3_kernel<2,2,2,2,1>[f16]"),
    "128-128 fold16 fat": (128, 128, 1, True, "relu6", 0, 3, [(20, 24), (24, 33)], 1, "conv3x3_kernel<4,2,2,2,1>[f16]"),      # (24 rows: the lower wave pair below the image)
    "128-256 ps_add": (128, 256, 1, False, "none", 1, 1, [(20, 24), (17, 21)], 0, "conv3x3_kernel<2,2,2,2,1>[f16]"),
    "128-256 ps_add fat": (128, 256, 1, False, "none", 1, 1, [(17, 20)], 1, "conv3x3_kernel<4,2,2,2,1>[f16]"),
    "64-128 stride 2": (64, 128, 2, False, "relu6", 0, 2, [(18, 36), (21, 37)], 0, "conv3x3_kernel<4,1,1,4,2>[f16]"),
    "64-64 fold8": (64, 64, 1, True, "relu6", 0, 3, [(20, 24), (21, 37)], 0, "conv3x3_kernel<2,2,4,1,1>[f16][fold8]"),
    # widths off the power-of-two grid (tests/test_gpu_widths.py): partly live channel tiles and granules, 3 / 5 / 24 chunks, Cout / 4 = 48
    "48-48": (48, 48, 1, False, "relu6", 0, 2, [(21, 37)], 0, "conv3x3_kernel<4,1,2,2,1>[f16]"),
    "128-192": (128, 192, 1, False, "relu6", 0, 2, [(20, 24)], 0, "conv3x3_kernel<2,2,2,2,1>[f16]"),
    "128-192 fat": (128, 192, 1, False, "relu6", 0, 2, [(20, 24)], 1, "conv3x3_kernel<4,2,2,2,1>[f16]"),
    "80-64 stride 2": (80, 64, 2, False, "relu6", 0, 2, [(18, 36)], 0, "conv3x3_kernel<4,1,1,4,2>[f16]"),
    "128-192 ps_add": (128, 192, 1, False, "none", 1, 1, [(17, 21)], 0, "conv3x3_kernel<2,2,2,2,1>[f16]"),
    "384-384 fold48": (384, 384, 1, True, "relu6", 0, 3, [(10, 19)], 0, "conv3x3_kernel<2,2,2,2,1>[f16]"),
    "384-384 fold48 fat": (384, 384, 1, True, "relu6", 0, 3, [(10, 19)], 1, "conv3x3_kernel<4,2,2,2,1>[f16]"),      # (the zero-chunk skip: 3 chunks per absent source)
}


@pytest.mark.parametrize("family", list(DIRECT))
def test_direct_form(family):
    from bsvd_amd.netspec import ConvSpec
    cin, cout, stride, tsm, act, epi, T, sizes, fat, variant = DIRECT[family]
    sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
    rs = np.random.RandomState(len(family) * 17 + cin + cout)
    st = _state(sp, rs)
    w, b = st["l.weight"], st["l.bias"]
    w_hi = S.pairs(w)[0]
    e1, e3 = _execs(_Net(sp), st, fat=fat)
    for H, W in sizes:
        xh, xl = _halves("canonical", (T, H, W, cin), rs)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        kw, extra_dev, extra_hi_dev = {}, None, None
        if epi == 1:          # the skip tensor: read as FULL pairs, real lo halves
            eh, el = _halves("canonical", (T, 2 * Ho, 2 * Wo, cout // 4), rs)
            kw = dict(extra=eh + el, extra_pstride=cout // 4, extra_cstride=1)
            extra_dev, extra_hi_dev = S.container(eh, el).to(_dev()), S.container(eh, np.zeros_like(el)).to(_dev())
        ekw = (extra_dev, kw.get("extra_pstride", 0), kw.get("extra_cstride", 1))
        for tag, hp, hn in _halo_forms(sp, "canonical", T, H, W, rs):
            model = F.direct_one_pass(sp, xh, xl, w, b, hp, hn, **kw)
            err = S.chain_err(sp, xh, w_hi, b, halo_prev=S._h(hp, 0), halo_next=S._h(hn, 0), **kw)
            got = e1.conv(sp, S.container(xh, xl).to(_dev()), _halo(hp, "real"), _halo(hn, "real"), *ekw)
            assert e1.last_variant == variant, e1.last_variant
            gh, gl = S.halves(got.cpu())
            need = S.needed(gh + gl, model, err)
            _report("%s %dx%d | %s" % (family, H, W, tag), need, F.M_DIRECT, err, float(model.abs().max()))
            assert float(model.abs().max()) > 0.1 and need <= F.M_DIRECT, (family, H, W, tag, need)                  # (a)
            ref3 = e3.conv(sp, S.container(xh, np.zeros_like(xl)).to(_dev()), _halo(hp, "zero"), _halo(hn, "zero"), *ekw)
            assert e3.last_variant == variant.replace("[f16]", "[f16x3]"), e3.last_variant
            assert _values_equal(got, ref3), (family, H, W, tag, "one pass != three passes with x_lo = 0, w_lo = 0")     # (b)
            nan = e1.conv(sp, _cont(xh).to(_dev()), _halo(hp, "nan"), _halo(hn, "nan"), *ekw)
            assert np.isfinite(sum(S.halves(nan.cpu()))).all()
            assert _values_equal(nan, ref3), (family, H, W, tag, "a lo half reached an MFMA operand")                   # (c)
            if epi == 1 and tag == "no halo":
                # the skip operand keeps its real lo halves and they COUNT: (a) above held the result to the model on decoded full pairs;
                # without them the result moves by what they carry
                no_lo = e1.conv(sp, S.container(xh, xl).to(_dev()), None, None, extra_hi_dev, ekw[1], ekw[2])
                d = torch.as_tensor(sum(S.halves(got.cpu())) - sum(S.halves(no_lo.cpu()))).abs().max()
                assert 0 < float(d) < 2.0 ** -9 and not _values_equal(got, no_lo)


@pytest.mark.parametrize("H,W", [(20, 24), (21, 37)])
def test_planar_exit_with_a_split_base(H, W):
    """64 -> 3 RESID, planar fp32 output; the residual base is an engine tensor decoded from FULL pairs (BsvdConvArgs.extra_split)"""
    from bsvd_amd.netspec import ConvSpec
    T = 2
    rs = np.random.RandomState(H + W)
    sp = ConvSpec("l", "l", 64, 3, 1, False, "none", 2)
    st = _state(sp, rs)
    w, b = st["l.weight"], st["l.bias"]
    e1, e3 = _execs(_Net(sp), st)
    xh, xl = _halves("canonical", (T, H, W, 64), rs)
    eh, el = _halves("canonical", (T, H, W, 64), rs)
    kw = dict(extra=eh + el, extra_pstride=64, extra_cstride=1)
    base, base_hi = S.container(eh, el).to(_dev()), S.container(eh, np.zeros_like(el)).to(_dev())
    for clamp in (None, (0.0, 1.0)):
        run = lambda e, x, bs=base: e.conv(sp, x.to(_dev()), extra=bs, extra_pstride=64, extra_cstride=1, y_planar=(3, clamp))
        model = F.direct_one_pass(sp, xh, xl, w, b, y_planar=(3, clamp), **kw)
        err = S.chain_err(sp, xh, S.pairs(w)[0], b, y_planar=(3, clamp), **kw)
        got = run(e1, S.container(xh, xl))
        assert e1.last_variant == "conv3x3_kernel<2,1,4,1,1>[f16][planar out]" and got.shape == (T, 3, H, W), e1.last_variant
        need = S.needed(got.cpu(), model, err)
        _report("planar exit split base %dx%d | clamp %s" % (H, W, clamp), need, F.M_DIRECT, err, float(model.abs().max()))
        assert need <= F.M_DIRECT, need                                                                                  # (a)
        ref3 = run(e3, S.container(xh, np.zeros_like(xl)))
        assert "[f16x3][planar out]" in e3.last_variant
        assert np.array_equal(got.cpu().numpy(), ref3.cpu().numpy())                                                     # (b)
        nan = run(e1, _cont(xh))
        assert bool(torch.isfinite(nan).all()) and np.array_equal(nan.cpu().numpy(), ref3.cpu().numpy())                 # (c)
        # the residual base keeps its real lo halves, and they count
        no_lo = run(e1, S.container(xh, xl), base_hi)
        if clamp is None:
            assert 0 < float((got - no_lo).abs().max()) < 2.0 ** -9


@pytest.mark.parametrize("cin,cmid,cout,act,T,H,W", [(4, 64, 64, "relu6", 2, 20, 24), (4, 64, 64, "relu6", 1, 21, 37), (3, 30, 64, "relu", 2, 17, 21)])
def test_fused_entry(cin, cmid, cout, act, T, H, W):
    """BsvdConvArgs.head_w_packed under BSVD_F16: one pass in the first conv's small GEMM AND in the main K loop.  x and the first conv's
    weights and bias sit on dyadic grids (2^-6, 2^-8): the middle tensor is exact in fp32, see the module docstring."""
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import ConvSpec

    class Net:
        pass

    rs = np.random.RandomState(cin + cmid + H)
    sp0 = ConvSpec("inc0", "b.inc.convblock.0", cin, cmid, 1, False, act, 0)
    sp3 = ConvSpec("inc3", "b.inc.convblock.3", cmid, cout, 1, False, act, 0)
    net = Net()
    net.layers, net.temp1 = [sp0, sp3], {"inc0": sp0, "inc3": sp3}
    st = {k: v for k, v in _state(sp3, rs).items() if k.startswith(sp3.key + ".")}
    st[sp0.key + ".weight"] = (rs.randint(-96, 97, (cmid, cin, 3, 3)) / 256.0).astype(np.float32)
    st[sp0.key + ".bias"] = (rs.randint(-64, 65, cmid) / 256.0).astype(np.float32)
    x = (np.round(np.clip(rs.standard_normal((T, cin, H, W)), -3, 3) * 64) / 64).astype(np.float32)
    ex = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16"))
    assert ex.fuse_head(net.temp1)
    xn = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float64)
    w0, b0, w3, b3 = (st[sp0.key + ".weight"], st[sp0.key + ".bias"], st[sp3.key + ".weight"], st[sp3.key + ".bias"])
    assert np.array_equal(S.pairs(w0)[0], w0) and np.array_equal(S.fp16(xn), xn)
    mid = F.direct_one_pass(sp0, xn, None, w0, b0)[..., :cmid]
    assert np.array_equal(mid.numpy().astype(np.float32).astype(np.float64), mid.numpy())          # exact in fp32
    pad = lambda t: np.concatenate([t, np.zeros(t.shape[:-1] + (sp3.cin_pad - cmid,))], axis=-1)
    mh = pad(S.pairs(mid)[0])
    model = F.direct_one_pass(sp3, mh, None, w3, b3)
    err = S.chain_err(sp3, mh, S.pairs(w3)[0], b3)
    ex.record_variants = True
    got = ex.conv_head_fused(sp0, sp3, torch.from_numpy(x).to(_dev()))
    assert ex.last_variant == "conv3x3_kernel<4,1,2,2,1>[f16][fused entry]", ex.last_variant
    need = S.needed(sum(S.halves(got.cpu())), model, err)
    _report("fused entry %d-%d-%d %dx%d" % (cin, cmid, cout, H, W), need, F.M_DIRECT, err, float(model.abs().max()))
    assert float(model.abs().max()) > 0.1 and need <= F.M_DIRECT, need                                                # (a)
    # (c) the planar input is split inside the kernel: what lies below fp16(x) must not count.  (There is no (b) here: the three-pass
    #     kernel re-splits the middle tensor and its main conv reads that lo.)
    x2 = rs.standard_normal((T, cin, H, W)).astype(np.float32)
    a = ex.conv_head_fused(sp0, sp3, torch.from_numpy(x2).to(_dev()))
    c = ex.conv_head_fused(sp0, sp3, torch.from_numpy(x2).half().float().to(_dev()))
    assert torch.equal(a, c) and np.isfinite(sum(S.halves(a.cpu()))).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Winograd F(2,3)

def _grid_pair(shape, rs, kind):
    """(decoded x, (hi, lo)): 'lo0' -- x on the 2^-6 grid below 3, lo = 0; 'noncanon' -- hi' = hi - d, lo' = lo + d with hi on the 2^-6 grid, lo on
    the 2^-10 grid below 2^-7, d on the 2^-6 grid below 1: not a canonical pair, every half an fp16 value, hi + lo exact in fp32 (12 bits).
    Differences of two such x (F(2,3)'s BT) are exact in fp32."""
    hi = np.round(np.clip(rs.standard_normal(shape), -3, 3) * 64) / 64
    if kind == "lo0":
        return hi, (hi, np.zeros_like(hi))
    lo = rs.randint(-7, 8, shape) / 1024.0
    d = rs.randint(-63, 64, shape) / 64.0
    return hi + lo, (hi - d, lo + d)


WINO = {
    # name: (cin, cout, tsm, act, epi, T)
    "128-128 fold16": (128, 128, True, "relu6", 0, 3),
    "256-256 fold32": (256, 256, True, "relu", 0, 2),
    "128-256 ps_add": (128, 256, False, "none", 1, 1),
    "128-192": (128, 192, False, "relu", 0, 2),              # the second 128-channel tile half live
    "384-384 fold48": (384, 384, True, "relu6", 0, 2),       # 24 chunks, three per temporal source, three channel tiles
}


@pytest.mark.parametrize("H", [9, 20])          # 20 rows: a 16-row grid whose last band (4 live rows) is the folded one
@pytest.mark.parametrize("kind", ["lo0", "noncanon"])
@pytest.mark.parametrize("layer", list(WINO))
def test_wino_f23(layer, kind, H):
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    cin, cout, tsm, act, epi, T = WINO[layer]
    W = 22
    rs = np.random.RandomState(cin + cout + H + len(kind))
    sp = ConvSpec("l", "l", cin, cout, 1, tsm, act, epi)
    st = _state(sp, rs, wino_m=2)
    w, b = st["l.weight"], st["l.bias"]
    e1, _ = _execs(_Net(sp), st, "wino2")
    assert "l" in e1.packed.wino
    x, xc = _grid_pair((T, H, W, cin), rs, kind)
    kw, extra_dev = {}, None
    if epi == 1:          # skip tensor: full canonical pairs
        eh, el = _halves("canonical", (T, 2 * H, 2 * W, cout // 4), rs)
        kw = dict(extra=eh + el, extra_pstride=cout // 4, extra_cstride=1)
        extra_dev = S.container(eh, el).to(_dev())
    forms = [("no halo", None, None, None, None)]
    if tsm:
        f = sp.fold
        p, pc = _grid_pair((H, W, f), rs, kind)
        n, nc = _grid_pair((H, W, f), rs, kind)
        forms.append(("compact", (p, f, 0), (n, f, 0), (pc, f, 0), (nc, f, 0)))
        fr, fc = _grid_pair((1, H, W, cin), rs, kind)
        forms.append(("full frame", (fr, cin, f), (fr, cin, 0), (fc, cin, f), (fc, cin, 0)))
    seen = set()
    for tag, hp, hn, hpc, hnc in forms:
        mh = lambda h: None if h is None else Halo(h[0], h[1], h[2])
        model = F.wino_one_pass(sp, x, w, 2, b, mh(hp), mh(hn), **kw)
        err = S.wino_err(sp, x, w, 2, b, halo_prev=mh(hp), halo_next=mh(hn), **kw)
        assert float(model.abs().max()) > 0.1
        for xf in (False, True):          # input as pairs / as plain fp32 (BsvdConvArgs.x_f32)
            dv = (lambda v, c: torch.from_numpy(v.astype(np.float32)).to(_dev())) if xf else (lambda v, c: S.container(*c).to(_dev()))
            dh = lambda h, c: None if h is None else Halo(dv(h[0], c[0]), h[1], h[2])
            xd, hpd, hnd = dv(x, xc), dh(hp, hpc), dh(hn, hnc)
            for yf in (False, True):      # output as pairs / as plain fp32 (BsvdConvArgs.y_f32)
                e1.force_x_f32, e1.force_y_f32 = xf, yf
                outs = []
                for code in (2, 42):      # the kernel picks its tile (these grids: the 8-row one) / never the half-height tile (16 rows, folded band)
                    a, y = e1.build_args(sp, xd, hpd, hnd, extra_dev, kw.get("extra_pstride", 0), kw.get("extra_cstride", 1))
                    a.wino_m = code
                    buf = ctypes.create_string_buffer(96)
                    assert e1.lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96) == 0
                    name = buf.value.decode()
                    assert name.startswith("winox_kernel<F(2,3),2x2>[f16]") and ("[f32 in]" in name) == xf, name
                    assert e1.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
                    seen.add(name)
                    outs.append(y)
                    val = y.cpu().double() if yf else sum(S.halves(y.cpu()))
                    need = S.needed(val, model, err)
                    _report("wino2 %s H=%d %s | %s%s | %s" % (layer, H, kind, name[name.index("]") + 1:] or "[16 rows]", "[f32 out]" if yf else "", tag),
                            need, F.M_WINO2, err, float(model.abs().max()))
                    assert need <= F.M_WINO2, (layer, kind, H, tag, name, yf, need)                                       # (a), (c)
                assert torch.equal(outs[0], outs[1]), (layer, kind, H, tag, xf, yf, "tile variants differ")                 # (b)
    assert any("[8 rows]" in n for n in seen) and any("[8 rows]" not in n for n in seen), seen


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals on the device path

def test_refusals_return_their_code_and_launch_nothing():
    from bsvd_amd import _lib
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import ConvSpec
    from test_gpu_pair import _PairNet
    rs = np.random.RandomState(1)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(ex, a, y, what):
        y.fill_(12345.0) if isinstance(y, torch.Tensor) else y.t.fill_(12345.0)
        a.dtype = _lib.BSVD_F16
        rc = ex.lib.bsvd_conv3x3(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        msg = ex.lib.bsvd_last_error().decode()
        t = y if isinstance(y, torch.Tensor) else y.t
        assert rc == -24 and "BSVD_F16" in msg and what in msg and bool((t == 12345.0).all()), (rc, msg)

    # fused pair
    a_, b_ = ConvSpec("out0", "a", 64, 64, 1, False, "relu6", 0), ConvSpec("out3", "b", 64, 64, 1, False, "relu6", 0)
    st = seeded_state([("e0.weight", (16, 4, 3, 3)), ("e0.bias", (16,)), ("e1.weight", (3, 16, 3, 3)), ("e1.bias", (3,))], 5)
    for sp in (a_, b_):
        st.update({k: v for k, v in _state(sp, rs).items() if k.startswith(sp.key + ".")})
    net = _PairNet(a_, b_)
    ex = HipExecutor(PackedNet(net, {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3", "direct", fuse_pairs=True))
    x = S.container(*_halves("canonical", (1, 20, 24, 64), rs)).to(_dev())
    a, y = ex.build_args(b_, x, pre=a_)
    refused(ex, a, y, "pre_w_packed")
    # F(6,3) and the transformed-domain hand-over
    sp = ConvSpec("l", "l", 128, 128, 1, False, "relu6", 0)
    st = _state(sp, rs, wino_m=6)
    ex = HipExecutor(PackedNet(_Net(sp), {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16x3", "wino6"))
    x = S.container(*_halves("canonical", (1, 9, 22, 128), rs)).to(_dev())
    ex.force_x_f32 = ex.force_y_f32 = False
    a, y = ex.build_args(sp, x)
    refused(ex, a, y, "wino_m 6")
    ex.force_y_v = 6
    a, y = ex.build_args(sp, x)
    assert a.y_v == 6
    refused(ex, a, y, "y_v")
    # ... and through the package: the combinations never reach the library
    with pytest.raises(ValueError, match="f16"):
        PackedNet(_Net(sp), {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16", "wino6")


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole networks

NETS = {
    "c32": dict(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32),
    "c64": dict(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64),
    "blind": dict(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu", interm_ch=30, blind=True),
}
_CACHE = {}


def _model(name, st, **kw):
    import bsvd_amd
    m = bsvd_amd.BSVD(pretrain_ckpt=None, precision="f16", **dict(NETS[name], **kw))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    return m.to(_dev()).eval()


def _net_case(name):
    """per network, computed once: weights, clip, the fp32 CPU oracle, the CPU emulation of the mode, the GPU clip result"""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import bsvd_oracle as O
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import bsvd_clip
    c = NETS[name]
    blind = c.get("blind", False)
    st = seeded_state(bsvd_keys(c["chns"], c["mid_ch"], c["in_ch"], c["out_ch"], c["interm_ch"], blind), 11)
    rs = np.random.RandomState(5)
    T, H, W = 5, 32, 48
    cin = 3 if blind else 4
    x = rs.uniform(0, 1, (T, cin, H, W)).astype(np.float32)
    if not blind:
        x[:, 3] = 30 / 255.0
    x = torch.from_numpy(x)
    net = make_netspec(c["chns"], c["mid_ch"], c["in_ch"], c["out_ch"], c["act"], c["interm_ch"], blind=blind)
    from oracle_exec import OracleExecutor
    want = bsvd_clip(OracleExecutor(st, double=True), net, x, x_planar=True, y_planar=(net.out_ch, None))
    emu = bsvd_clip(F.F16EmuExecutor(st), net, x, x_planar=True, y_planar=(net.out_ch, None))
    m = _model(name, st)
    got = m.clip_forward(x.to(_dev()))
    _CACHE[name] = dict(st=st, x=x, want=want, emu=emu, m=m, got=got)
    return _CACHE[name]


def _per_frame(m, x):
    outs = [m.feedin_one_element(x[i:i + 1]) for i in range(x.shape[0])]
    while len(outs) < x.shape[0] + m.shift_num:
        outs.append(m.feedin_one_element(None))
    assert m.feedin_one_element(None) is None
    m.reset()
    return torch.cat(outs[m.shift_num:])


@pytest.mark.parametrize("name", list(NETS))
def test_network_schedules_agree_bit_for_bit(name):
    c = _net_case(name)
    m, want = c["m"], c["got"]
    x = c["x"].to(_dev())
    assert m.precision == "f16" and m._executor(_dev()).mfma_dtype == 3
    for rep in range(3):              # batched launches, graph capture, graph replay
        assert torch.equal(_per_frame(m, x), want), (name, "per-frame stream", rep)
        for chunk in (1, "auto", 3):
            m.stream_chunk = chunk
            assert torch.equal(m.streaming_forward(x), want), (name, "chunked stream", chunk, rep)
    stt = m._stream_eng.stats
    assert stt["graph_captures"] > 0 and stt["graph_replays"] > 0
    m.stream_overlap = False          # not lagged: one chain per step
    assert torch.equal(m.streaming_forward(x), want)
    m.stream_overlap = True


@pytest.mark.parametrize("name", list(NETS))
def test_network_two_shards_equal_the_whole_clip(name):
    from bsvd_amd.dist import shard_range
    from bsvd_amd.schedule import Halo
    c = _net_case(name)
    x, T = c["x"].to(_dev()), c["x"].shape[0]
    world, boxes, results, errors = 2, {}, [None, None], []
    barrier = threading.Barrier(world)

    def rank(r):
        try:
            torch.cuda.set_device(0)
            m = _model(name, c["st"])
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
    assert torch.equal(torch.cat(results), c["got"])


@pytest.mark.parametrize("name", list(NETS))
def test_network_error_within_twice_the_emulations(name):
    c = _net_case(name)
    e_emu = float((c["emu"].double() - c["want"].double()).abs().max())
    e_gpu = float((c["got"].cpu().double() - c["want"].double()).abs().max())
    ms = _model(name, c["st"], weight_scale="auto")
    e_ws = float((ms.clip_forward(c["x"].to(_dev())).cpu().double() - c["want"].double()).abs().max())
    assert ms._executor(_dev()).packed.scale_exp
    print("NET | %s | max-abs vs the fp32 CPU oracle: emulation %.3e, MI355X %.3e (%.2f x), with weight_scale='auto' %.3e (%.2f x)"
          % (name, e_emu, e_gpu, e_gpu / e_emu, e_ws, e_ws / e_emu))
    assert e_emu > 1e-5                                  # fp16-class: the emulation itself is far from the 3-pass mode's 2-7e-5 ... on O(1) outputs
    assert e_gpu <= 2 * e_emu, (name, e_gpu, e_emu)
    assert e_ws <= 2 * e_emu, (name, e_ws, e_emu)


def test_psnr_parity_proxy_within_0p02_db():
    """tests/test_gpu_eval.py::test_psnr_parity_proxy_within_0p02_db restated for precision='f16': the project's condition for offering a mode to
    reference users.  (The CPU emulation of the mode on this clip: profiles/f16_one_pass.txt.)"""
    import bsvd_amd
    from oracle import bsvd_oracle as O
    from bsvd_amd import evaluation as E
    rs = np.random.RandomState(8)
    T, H, W = 4, 96, 128
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.stack([np.stack([0.5 + 0.4 * np.sin(0.07 * (xx + 3 * t) + c) * np.cos(0.05 * yy + 0.3 * c) for c in range(3)])
                   for t in range(T)]).astype(np.float32)
    lq = gt + rs.standard_normal(gt.shape).astype(np.float32) * np.float32(30 / 255.0)
    x = torch.from_numpy(np.concatenate([lq, np.full((T, 1, H, W), 30 / 255.0, np.float32)], axis=1))[None]
    st = seeded_state(bsvd_keys([64, 128, 256], 64, 4, 3, 64), 11)
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64,
                      pretrain_ckpt=None, precision="f16")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    got = torch.clamp(m.to(_dev())(x.to(_dev())).cpu()[0], 0, 1)
    want = torch.clamp(O.bsvd_clip(x, O.to_torch_state(st))[0], 0, 1)
    clean = torch.from_numpy(gt)
    worst = [0.0, 0.0]
    for f in range(T):
        d_u8 = (E.calculate_psnr(E.tensor2img(got[f]), E.tensor2img(clean[f]), 2) - E.calculate_psnr(E.tensor2img(want[f]), E.tensor2img(clean[f]), 2))
        d_fl = (E.calculate_psnr_float(got[f], clean[f], 2) - E.calculate_psnr_float(want[f], clean[f], 2))
        worst = [max(worst[0], abs(d_u8)), max(worst[1], abs(d_fl))]
    print("PSNR | f16 | worst |d PSNR| over %d frames: uint8-domain %.5f dB, float %.5f dB; max-abs vs the oracle %.3e"
          % (T, worst[0], worst[1], float((got - want).abs().max())))
    assert worst[0] < 0.02 and worst[1] < 0.02, worst
