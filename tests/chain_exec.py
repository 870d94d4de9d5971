"""Executor on the CPU model of the exact-fp32 mode (oracle/chain_ref.c) for TESTS ONLY.

The interface of oracle_exec.OracleExecutor (so bsvd_amd.schedule runs on it unchanged), the arithmetic of include/bsvd_hip.h's "Arithmetic of
BSVD_F32": one fmaf per term in a stated order, one fp32 operation per epilogue step.  What it returns is what a kernel of that mode must
return BIT FOR BIT (tests/test_gpu_fp32_chain.py); the order is chosen per kernel family exactly as the library chooses the kernel:
a planar input runs the entry kernel, a planar output the exit kernel, everything else the MFMA kernel.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from bsvd_amd.netspec import EPI_PS_ADD, EPI_RESID
from oracle import chain_ref as CR
from oracle_exec import OracleExecutor, _slice_from_halo

# family -> (order, flags) of the chain that the header documents for it
CHAIN_OF = {
    "mfma": (CR.ORDER_MFMA, 0),
    "head": (CR.ORDER_EDGE, CR.BIAS_FIRST),
    "tail": (CR.ORDER_EDGE, 0),
}


def family_of(x_planar, y_planar):
    return "head" if x_planar else ("tail" if y_planar is not None else "mfma")


def bits(a):
    """fp32 bit patterns with -0 mapped to +0 (the chain's zero-operand terms and a kernel that skips them differ in nothing else)"""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    return (a + np.float32(0.0)).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def assert_same_bits(got, want, what=""):
    """What tests/test_gpu_fp32_chain.py and the tightened parity tests assert of a kernel's result: no NaN, and the model's bits"""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert not np.isnan(g).any(), "%s: NaN in the result" % what
    bad = bits(g) != bits(w)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ in their bits, max-abs %.3e; first at %s: got %r (0x%08x), model %r (0x%08x)"
                             % (what, int(bad.sum()), bad.size, float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()), i,
                                float(g[i]), int(bits(g)[i]), float(w[i]), int(bits(w)[i])))


class ChainExecutor(OracleExecutor):
    def __init__(self, state, chain_of=None, flags=0):
        """chain_of: override of CHAIN_OF (family -> (order, flags)); flags: OR-ed into every layer's flags (the CPU tests' mutations)"""
        super().__init__(state)
        self.chain_of = dict(CHAIN_OF, **(chain_of or {}))
        self.flags = flags

    def conv(self, sp, x, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1,
             x_planar=False, y_planar=None, out=None):
        if out is not None:
            out.copy_(self.conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar))
            return out
        self.launches += 1
        self.log.append(sp.key)
        if x_planar:
            T, C, H, W = x.shape
            assert C == sp.cin and sp.cin_pad == 16
            v = x.contiguous()
        else:
            T, H, W, cp = x.shape
            assert cp == sp.cin_pad, (sp.key, cp, sp.cin_pad)
            assert float(x[..., sp.cin:].abs().max()) == 0.0 if cp > sp.cin else True, "padded input channels must be zero"
            v = x[..., :sp.cin].permute(0, 3, 1, 2).contiguous()       # [T,cin,H,W]
        fold = sp.fold if sp.tsm else 0
        Ho, Wo = (H - 1) // sp.stride + 1, (W - 1) // sp.stride + 1
        order, flags = self.chain_of[family_of(x_planar, y_planar)]
        w, b = self.state[sp.key + ".weight"].numpy(), self.state[sp.key + ".bias"].numpy()
        e = None
        if extra is not None and sp.epilogue in (EPI_PS_ADD, EPI_RESID):
            ef = extra.reshape(-1)
            if sp.epilogue == EPI_PS_ADD:
                npix, k = 4 * Ho * Wo, sp.cout // 4
                eh, ew = 2 * Ho, 2 * Wo
            else:
                npix, k = Ho * Wo, min(3, sp.cout)
                eh, ew = Ho, Wo
            e = torch.as_strided(ef, (T, npix, k), (extra[0].numel(), extra_pstride, extra_cstride), storage_offset=ef.storage_offset())
            e = e.reshape(T, eh, ew, k).permute(0, 3, 1, 2).contiguous().numpy()          # [T,k,eh,ew]
        clamp = None if y_planar is None else y_planar[1]
        ys = []
        for t in range(T):
            prev_sl = next_sl = None
            if fold:
                if t > 0:
                    prev_sl = v[t - 1, fold:2 * fold].numpy()
                elif halo_prev is not None:
                    prev_sl = _slice_from_halo(halo_prev, H * W, fold).t().reshape(fold, H, W).contiguous().numpy()
                if t + 1 < T:
                    next_sl = v[t + 1, :fold].numpy()
                elif halo_next is not None:
                    next_sl = _slice_from_halo(halo_next, H * W, fold).t().reshape(fold, H, W).contiguous().numpy()
            ys.append(CR.conv3x3(v[t].numpy(), w, b, prev_sl, next_sl, fold, sp.stride, sp.act, sp.epilogue, None if e is None else e[t],
                                 resid_ch=3, clamp=clamp, order=order, flags=flags | self.flags))
        y = torch.from_numpy(np.stack(ys))                                                # NCHW
        if y_planar is not None:
            assert y_planar[0] == sp.cout
            return y
        cpad = sp.cout_pad // 4 if sp.epilogue == EPI_PS_ADD else sp.cout_pad
        res = torch.zeros((T,) + tuple(y.shape[-2:]) + (cpad,), dtype=torch.float32)
        res[..., :y.shape[1]] = y.permute(0, 2, 3, 1)
        return res


# ------------------------------------------------------------------------------------------------ the cases both chain test files share
# One layer, one kernel family of the exact-fp32 mode.  kind: "layer" (NHWC in and out), "head" (planar entry), "tail" (planar exit).
# halos: "none" | "compact" | "full"; extra: None | "skip" (PS_ADD) | "planar" | "nhwc" (RESID base); generic: reach the [generic] kernel through
# an x that is not 16-byte aligned (a fold that is no multiple of 4 gets there by itself); expect: what bsvd_conv3x3_variant must name.
Case = namedtuple("Case", "name kind cin cout stride tsm act epi T H W halos extra clamp tile_order generic expect")

NARROW, WIDE, FOLD8, STRIDE2 = "conv3x3_kernel<2,2,4,1,1>[f32]", "conv3x3_kernel<2,2,2,2,1>[f32]", "[fold8]", "conv3x3_kernel<2,2,2,2,2>[f32]"


def _L(name, cin, cout, stride, tsm, act, epi, T, H, W, halos="none", extra=None, order=0, generic=False, expect=""):
    return Case(name, "layer", cin, cout, stride, tsm, act, epi, T, H, W, halos, extra, None, order, generic, expect)


def _H(name, cin, cout, act, T, H, W):
    return Case(name, "head", cin, cout, 1, False, act, 0, T, H, W, "none", None, None, 0, False, "head_kernel<%d>" % cin)


def _T(name, cin, cout, act, epi, T, H, W, extra, clamp):
    return Case(name, "tail", cin, cout, 1, False, act, epi, T, H, W, "none", extra, clamp, 0, False, "tail_kernel<%d>" % (3 if cout == 3 else 4))


# Tiles: <2,2,4,1,1> 16 x 16 pixels, <2,2,2,2,1> and the stride-2 tile 8 x 16 output pixels, head 4 x 64, tail 32 x 16.  17 x 33 is a full tile
# plus a ragged one in both directions for the MFMA tiles (stride 2: 27 x 43 -> 14 x 22); the entry and exit kernels get 5 x 70 and 33 x 17
# on top of the shapes the other families use, because their tiles are 64 wide resp. 32 high.
FAMILY_CASES = [
    # ---- Cout <= 64
    _L("narrow 64 relu6", 64, 64, 1, False, "relu6", 0, 1, 17, 33, expect=NARROW),
    _L("narrow 30->32 relu, order 1", 30, 64, 1, False, "relu", 0, 1, 9, 17, order=1, expect=NARROW),
    _L("narrow 3->16 none, 3 frames", 3, 32, 1, False, "none", 0, 3, 20, 36, expect=NARROW),
    _L("narrow 1x1", 64, 64, 1, False, "relu6", 0, 1, 1, 1, expect=NARROW),
    _L("narrow RESID, NHWC base", 64, 64, 1, False, "none", 2, 2, 17, 33, extra="nhwc", expect=NARROW),
    _L("narrow RESID, planar base, Cout 3", 64, 3, 1, False, "none", 2, 1, 9, 17, extra="planar", order=1, expect=NARROW),
    _L("narrow [generic], unaligned x", 64, 64, 1, False, "relu6", 0, 1, 17, 33, generic=True, expect=NARROW),
    _L("narrow [generic], fold 3, 3 frames, compact halos", 24, 40, 1, True, "relu6", 0, 3, 9, 17, "compact", generic=True, expect=NARROW),
    # ---- Cout > 64
    _L("wide 128, full halos", 128, 128, 1, True, "relu6", 0, 3, 9, 17, "full", expect=WIDE),
    _L("wide 256, K 2304, compact halos, order 1", 256, 256, 1, True, "relu", 0, 1, 9, 17, "compact", order=1, expect=WIDE),
    _L("wide 128, no halos", 128, 128, 1, True, "none", 0, 1, 17, 33, expect=WIDE),
    _L("wide PS_ADD with skip", 128, 256, 1, False, "none", 1, 1, 9, 17, extra="skip", expect=WIDE),
    _L("wide PS_ADD without skip, K 2304, order 1", 256, 512, 1, False, "none", 1, 1, 9, 17, order=1, expect=WIDE),
    _L("wide 1x1, compact halos", 128, 128, 1, True, "relu6", 0, 1, 1, 1, "compact", expect=WIDE),
    _L("wide [generic], unaligned x", 128, 128, 1, True, "relu6", 0, 3, 9, 17, "full", generic=True, expect=WIDE),
    # ---- fold 8
    _L("fold8, 3 frames", 64, 64, 1, True, "relu6", 0, 3, 17, 33, expect=FOLD8),
    _L("fold8, compact halos, order 1", 64, 64, 1, True, "relu", 0, 1, 9, 17, "compact", order=1, expect=FOLD8),
    _L("fold8, full halos", 64, 64, 1, True, "none", 0, 1, 20, 36, "full", expect=FOLD8),
    _L("fold8 1x1, 3 frames", 64, 64, 1, True, "relu6", 0, 3, 1, 1, expect=FOLD8),
    _L("fold8 [generic], unaligned x", 64, 64, 1, True, "relu6", 0, 3, 9, 17, "full", generic=True, expect="conv3x3_kernel<2,2,4,1,1>[f32]"),
    # ---- stride 2
    _L("stride 2, 27x43", 64, 128, 2, False, "relu6", 0, 1, 27, 43, expect=STRIDE2),
    _L("stride 2, 128->256, order 1", 128, 256, 2, False, "relu", 0, 1, 20, 36, order=1, expect=STRIDE2),
    _L("stride 2, narrow Cout", 32, 64, 2, False, "none", 0, 3, 9, 17, expect=STRIDE2),
    _L("stride 2 1x1", 64, 128, 2, False, "relu6", 0, 1, 1, 1, expect=STRIDE2),
    _L("stride 2 [generic], unaligned x", 64, 128, 2, False, "relu6", 0, 1, 17, 33, generic=True, expect=STRIDE2),
    # ---- planar entry
    _H("head 4->64 relu6", 4, 64, "relu6", 2, 17, 33),
    _H("head 3->30 relu", 3, 30, "relu", 1, 9, 17),
    _H("head 4->32 none 1x1", 4, 32, "none", 3, 1, 1),
    _H("head 4->64, a full 64-wide tile", 4, 64, "relu6", 1, 5, 70),
    # ---- planar exit
    _T("tail 3, planar base, clamp", 64, 3, "none", 2, 2, 17, 33, "planar", (0.0, 1.0)),
    _T("tail 3, NHWC base", 64, 3, "none", 2, 1, 20, 36, "nhwc", None),
    _T("tail 4, planar base, relu", 64, 4, "relu", 2, 1, 9, 17, "planar", None),
    _T("tail 3 1x1, clamp", 32, 3, "none", 2, 1, 1, 1, "planar", (0.0, 1.0)),
    _T("tail 3, a full 32-high tile, NHWC base, clamp", 64, 3, "none", 2, 1, 33, 17, "nhwc", (0.0, 1.0)),
    _T("tail 4, 128 in, relu6, PLAIN", 128, 4, "relu6", 0, 1, 9, 17, None, None),
]


def spec_of(c):
    from bsvd_amd.netspec import ConvSpec
    sp = ConvSpec("l", "l", c.cin, c.cout, c.stride, c.tsm, c.act, c.epi)
    return SimpleNamespace(layers=[sp]), sp


def operands(c, data):
    """The CPU-side operands of case ``c``: (sp, net, state, x, kw) with kw the keywords of an executor's conv().
    data "normal": N(0,1) inputs and the seeded weights of test_gpu_parity.  data "integer": the exact-integer probe -- inputs odd integers,
    weights from {-2 .. 2}, bias and the epilogue's second operand integers with |.| <= 1000.  Inputs lie in [-2047, 2047] for Cin = 256 and in
    [-4095, 4095] for Cin <= 128: an odd integer below 2048 has 11 significant bits, so a kernel that carried its operands at fp16's or tf32's 11
    bits would pass a probe made of them alone; below 4096 it has 12, and the worst case is the same: every partial sum of every order is an
    integer below 256 * 9 * 2047 * 2 + 2000 resp. 128 * 9 * 4095 * 2 + 2000 = 9 436 880 < 2^24, exact in fp32 whatever the order
    (tests/test_fp32_chain_cpu.py proves it per case in int64).  ReLU6 layers: inputs scaled by 2^-20 (exact), so the sums sit around 0.1 and
    the outputs straddle 0 (bias 0) and 6 (bias 6); their bias is an integer in [-6, 6] -- in units of 2^-20 that is <= 6 291 456, and
    9 434 880 + 6 291 456 < 2^24 keeps acc + bias exact too."""
    from seeded import seeded_state
    from bsvd_amd.netspec import pad16
    from bsvd_amd.schedule import Halo
    net, sp = spec_of(c)
    rs = np.random.RandomState((c.cin * 1000 + c.cout * 7 + c.stride + c.H * 31 + c.W) % (2 ** 31))
    integer = data == "integer"
    assert c.cin <= 256 and not (integer and c.act == "relu6" and c.epi != 0)
    half = 1024 if c.cin > 128 else 2048
    scale = np.float32(2.0 ** -20) if integer and c.act == "relu6" else np.float32(1.0)

    def draw(*shape):
        if integer:
            return torch.from_numpy(((2 * rs.randint(-half, half, shape) + 1).astype(np.float32) * scale))
        return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))

    def draw_extra(*shape):
        if integer:
            return torch.from_numpy(rs.randint(-1000, 1001, shape).astype(np.float32))
        return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))

    if integer:
        bmax = 6 if c.act == "relu6" else 1000
        bias = rs.randint(-bmax, bmax + 1, (c.cout,)).astype(np.float32)
        if c.act == "relu6":
            bias[:2] = (0.0, 6.0)[:min(2, c.cout)]
        st = {"l.weight": rs.randint(-2, 3, (c.cout, c.cin, 3, 3)).astype(np.float32), "l.bias": bias}
    else:
        st = seeded_state([("l.weight", (c.cout, c.cin, 3, 3)), ("l.bias", (c.cout,))], 7)
    T, H, W = c.T, c.H, c.W
    Ho, Wo = (H - 1) // c.stride + 1, (W - 1) // c.stride + 1
    kw = {}
    if c.kind == "head":
        x = draw(T, c.cin, H, W)
        kw["x_planar"] = True
    else:
        x = torch.zeros((T, H, W, pad16(c.cin)))
        x[..., :c.cin] = draw(T, H, W, c.cin)
    if c.extra == "skip":
        cqp = sp.cout_pad // 4
        e = torch.zeros((T, 2 * Ho, 2 * Wo, cqp))
        e[..., :c.cout // 4] = draw_extra(T, 2 * Ho, 2 * Wo, c.cout // 4)
        kw.update(extra=e, extra_pstride=cqp, extra_cstride=1)
    elif c.extra == "nhwc":
        kw.update(extra=draw_extra(T, Ho, Wo, 64), extra_pstride=64, extra_cstride=1)
    elif c.extra == "planar":
        kw.update(extra=draw_extra(T, 4, Ho, Wo), extra_pstride=1, extra_cstride=Ho * Wo)
    if c.halos != "none":
        fold = sp.fold
        if c.halos == "compact":
            kw.update(halo_prev=Halo(draw(H, W, fold), fold, 0), halo_next=Halo(draw(H, W, fold), fold, 0))
        else:
            full = torch.zeros((1, H, W, pad16(c.cin)))
            full[..., :c.cin] = draw(1, H, W, c.cin)
            kw.update(halo_prev=Halo(full, pad16(c.cin), fold), halo_next=Halo(full, pad16(c.cin), 0))
    if c.kind == "tail":
        kw["y_planar"] = (c.cout, c.clamp)
    return sp, net, st, x, kw
